"""The YUV conversion's rules C1-C7 (csrc/yuv_core.h) without a GPU: the host build walks the device kernel's work items, every load and
store audited for bounds and alignment (tests/hostemu/emu_yuv.cpp), against the independent NumPy statement tests/yuv_ref.py."""
import ctypes as C
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import emu_yuv_api as emu
import emu_jpegdec_api as emu_jd
import yuv_ref as ref
from conftest import ROOT, load_pkg

GEOMETRIES = ((2, 2), (16, 2), (18, 4), (34, 6), (48, 8), (64, 2))
KINDS = ("tight", "odd", "wide", "tall")

# C4's known answers, (Y, U, V) -> (B, G, R)
KNOWN = (((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((128, 128, 128), (130, 130, 130)), ((81, 90, 240), (0, 0, 254)),
         ((145, 54, 34), (1, 255, 0)), ((41, 240, 110), (255, 0, 0)), ((0, 0, 0), (0, 154, 0)), ((255, 255, 255), (255, 125, 255)),
         ((1, 255, 0), (255, 54, 0)))


def vector_expected(fmt, w, L):
    """C7: 16-byte accesses need multiples of 16, I420's 8-byte chroma loads multiples of 8 (the pointers are the test's own, aligned)"""
    if w % 16 or L["frame_stride"] % 16 or L["y_offset"] % 16 or L["y_pitch"] % 16:
        return False
    if fmt in ("nv12", "nv21"):
        return L["u_offset"] % 16 == 0 and L["u_pitch"] % 16 == 0
    if fmt == "i420":
        return all(L[k] % 8 == 0 for k in ("u_offset", "u_pitch", "v_offset", "v_pitch"))
    return True


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("matrix", ref.MATRICES)
def test_every_triple(matrix):
    """All 256^3 (Y, U, V) through the host build's pixel function equal the reference; `full` is jd_colour itself on a sample."""
    u, v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    u, v = u.ravel(), v.ravel()
    for y in range(256):
        Y = np.full(u.shape, y, np.uint8)
        got = emu.colour(Y, u, v, matrix)
        want = ref.colour(Y, u, v, matrix)
        assert np.array_equal(got, want), (matrix, y, np.argwhere(got != want)[:3])
    if matrix == "full":   # the JPEG decoder's own colour stage on 4:4:4 planes of a 16x8 image: D8 through another door
        w, h = 16, 8
        planes = noise(3 * w * h, 5)
        bgr = emu_jd.colour(planes, w, h, 3, 1, 1)
        # a 4:4:4 frame's planes are [2 x 1 blocks][64] per component, rows of 16 samples
        Yp, Cb, Cr = (planes[c * w * h:(c + 1) * w * h].reshape(h, w) for c in range(3))
        assert np.array_equal(bgr, emu.colour(Yp, Cb, Cr, "full").reshape(h, w, 3))


def test_known_answers():
    yuv = np.array([k[0] for k in KNOWN], np.uint8)
    want = np.array([k[1] for k in KNOWN], np.uint8)
    assert np.array_equal(emu.colour(yuv[:, 0], yuv[:, 1], yuv[:, 2], "video"), want)
    assert np.array_equal(ref.colour(yuv[:, 0], yuv[:, 1], yuv[:, 2], "video"), want)


def test_default_layout_and_refusals():
    """C2: the header's tight layout is the reference's, and yuv_check refuses by name."""
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


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_geometries_and_layouts(fmt):
    """Every matrix, size and layout on random bytes, three frames: the host build's frames are the reference's byte for byte, every access
    lies inside the arrays of exactly the implied sizes and is aligned as its width demands, and the bytes around the destination stay."""
    seed = 0
    for matrix, (w, h), kind in itertools.product(ref.MATRICES, GEOMETRIES, KINDS):
        L = ref.layout(fmt, w, h, kind)
        p = emu.params(fmt, w, h, matrix, L)
        batch = 3
        seed += 1
        buf = noise(ref.source_bytes(fmt, w, h, L, batch), seed)
        want = ref.to_bgr(buf, fmt, w, h, L, matrix, batch)
        r = emu.run(buf, p, batch)
        tag = (fmt, matrix, w, h, kind)
        assert (r.outside, r.misaligned) == (0, 0) and r.guard_ok, tag
        assert np.array_equal(r.bgr, want), tag
        vector = vector_expected(fmt, w, L)
        assert r.vector == int(vector), tag
        assert (r.wide > 0) == vector and r.stores == (batch * w * h * 3 // 16 if vector else batch * w * h * 3), tag
        # the same bytes from a source and into a destination one byte off: the generic cells, the same frames
        r1 = emu.run(buf, p, batch, src_offset=1, dst_offset=1)
        assert (r1.vector, r1.outside, r1.misaligned, r1.wide) == (0, 0, 0, 0) and r1.guard_ok and np.array_equal(r1.bgr, want), tag


def test_vector_and_generic_paths_agree():
    """One picture at w = 48: tight (vector groups), the same rows at an odd pitch (generic cells) and the tight frame forced through the
    generic cells give equal pixels, in every format."""
    bgr = noise(3 * 8 * 48 * 3, 11).reshape(3, 8, 48, 3)
    for fmt, matrix in itertools.product(ref.FORMATS, ref.MATRICES):
        tight, odd = ref.layout(fmt, 48, 8, "tight"), ref.layout(fmt, 48, 8, "odd")
        a = emu.run(ref.from_bgr(bgr, fmt, tight), emu.params(fmt, 48, 8, matrix, tight), 3)
        b = emu.run(ref.from_bgr(bgr, fmt, odd, fill=0x5A), emu.params(fmt, 48, 8, matrix, odd), 3)
        c = emu.run(ref.from_bgr(bgr, fmt, tight), emu.params(fmt, 48, 8, matrix, tight), 3, path=0)
        assert (a.vector, b.vector, c.vector) == (1, 0, 0)
        assert np.array_equal(a.bgr, b.bgr) and np.array_equal(a.bgr, c.bgr), (fmt, matrix)
        # and the conversion is a colour conversion: close to the picture the planes were made from, where the chroma cells are flat.  Rounding
        # Y to a byte moves a channel by at most 0.5 * 1.164, rounding U and V by at most 0.5 * 2.018 (B), the output's own rounding by 0.5:
        # under 2.1 in all, so 3 bounds it
        flat = np.repeat(np.repeat(bgr[:, ::2, ::2], 2, 1), 2, 2)
        back = emu.run(ref.from_bgr(flat, fmt, tight), emu.params(fmt, 48, 8, "video", tight), 3).bgr
        assert np.abs(back.astype(int) - flat.astype(int)).max() <= 3, fmt


def test_yv12_is_i420_with_the_planes_exchanged():
    w, h = 34, 6
    L = ref.layout("i420", w, h)
    buf = noise(ref.source_bytes("i420", w, h, L, 2), 3)
    yv12 = dict(L, u_offset=L["v_offset"], v_offset=L["u_offset"])
    got = emu.run(buf, emu.params("i420", w, h, layout=yv12), 2).bgr
    swapped = buf.copy()
    nc = (w // 2) * (h // 2)
    for f in range(2):
        o = f * L["frame_stride"]
        swapped[o + L["u_offset"]:o + L["u_offset"] + nc] = buf[o + L["v_offset"]:o + L["v_offset"] + nc]
        swapped[o + L["v_offset"]:o + L["v_offset"] + nc] = buf[o + L["u_offset"]:o + L["u_offset"] + nc]
    assert np.array_equal(got, emu.run(swapped, emu.params("i420", w, h), 2).bgr)
    assert np.array_equal(got, ref.to_bgr(buf, "i420", w, h, yv12, batch=2))


def test_params_layout_three_ways(tmp_path):
    """adas_yuv_params as gcc compiles the public header, _lib.YuvParams, the core header's YuvGeom and the emulation's ctypes mirror."""
    load_pkg()
    L = importlib.import_module("adas_amd._lib")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "adas_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(adas_yuv_params));']
    for fname, _ in L.YuvParams._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(adas_yuv_params, %s));' % (fname, fname))
    lines += ['  printf("consts %d %d %d %d %d %d %d\\n", ADAS_YUV_NV12, ADAS_YUV_NV21, ADAS_YUV_I420, ADAS_YUV_YUYV, ADAS_YUV_UYVY, ADAS_YUV_MATRIX_VIDEO, '
              'ADAS_YUV_MATRIX_FULL);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    got = dict(l.split(" ", 1) for l in out)
    size, offsets = emu.params_layout()
    assert int(got["size"]) == C.sizeof(L.YuvParams) == C.sizeof(emu.Params) == size == 72
    assert [f for f, _ in L.YuvParams._fields_] == [f for f, _ in emu.Params._fields_]
    for fname, _ in L.YuvParams._fields_:
        assert int(got[fname]) == getattr(L.YuvParams, fname).offset == getattr(emu.Params, fname).offset == offsets[fname], fname
    assert got["consts"].split() == [str(L.YUV_FORMATS[f]) for f in ref.FORMATS] + [str(L.YUV_MATRICES[m]) for m in ref.MATRICES]
    assert L.YUV_FORMATS == emu.FORMATS and L.YUV_MATRICES == emu.MATRICES and L.YUV_LAYOUT_FIELDS == emu.FIELDS == ref.FIELDS


def bounds_cases():
    """(argument, fmt, matrix, w, h, batch, layout) of the bounds program's run: the geometry list, every format, layout and matrix."""
    out = []
    for fmt, (w, h), kind in itertools.product(ref.FORMATS, GEOMETRIES, KINDS):
        matrix = ref.MATRICES[len(out) % 2]
        L = ref.layout(fmt, w, h, kind)
        arg = ",".join(str(v) for v in [emu.FORMATS[fmt], emu.MATRICES[matrix], w, h, 2] + [L[k] for k in ref.FIELDS])
        out.append((arg, fmt, matrix, w, h, 2, L))
    return out


def test_bounds_program_reproduces_the_reference():
    """The stand-alone program (plain g++ -O1 here; the -fsanitize=address,undefined run is by hand): exact-size arrays, the
    checksum of the reference's frames."""
    exe = emu.build_bounds()
    cases = bounds_cases()
    out = subprocess.check_output([exe] + [c[0] for c in cases], text=True).strip().splitlines()
    assert len(out) == len(cases) + 1
    total = 0
    for i, (arg, fmt, matrix, w, h, batch, L) in enumerate(cases):
        x = (12345 + i + 1) & 0xFFFFFFFF
        n = ref.source_bytes(fmt, w, h, L, batch)
        src = np.empty(n, np.uint8)
        for j in range(n):
            x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
            src[j] = x >> 24
        bgr = ref.to_bgr(src, fmt, w, h, L, matrix, batch).ravel().astype(object)
        s = int(sum(int(b) * (j + 1) for j, b in enumerate(bgr))) & 0xFFFFFFFFFFFFFFFF
        words = out[i].split()
        assert words[0] == arg and int(words[3]) == n and int(words[5]) == batch * w * h * 3 and int(words[7]) == s, (arg, out[i])
        assert words[1] == ("vector" if vector_expected(fmt, w, L) else "generic"), out[i]
        total = (total * 31 + s) & 0xFFFFFFFFFFFFFFFF
    assert out[-1] == "checksum %d" % total
