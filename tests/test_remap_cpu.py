"""The rectification stage's rules U1-U6 (csrc/remap_core.h) without a GPU: the host build walks both device kernels' work items, every map
load and store audited for bounds, alignment and writing each byte exactly once (tests/hostemu/emu_remap.cpp), against the NumPy
restatement tests/remap_ref.py -- and the lens model against an independently associated float64 evaluation and a physical bound."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import emu_remap_api as emu
import remap_ref as ref
from conftest import ROOT, load_pkg

SRC_HW = (23, 29)                                   # a 29x23 source
DST_HWS = ((25, 36), (25, 37), (25, 38), (25, 39))  # widths 36..39: no tail, tails of 1, 2, 3; an odd height, so frames start on every byte phase
MODEL_HW = (48, 64)
MODEL_K = (40.0, 40.0, 31.5, 23.5)
MODEL_LENSES = ("barrel", "rational", "pincushion")


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def small_camera(dst_hw, lens, shift=0):
    """The bounds program's camera: both focal lengths 20, the centres in the middle of their images, map m's centre moved by m pixels"""
    return dict(K=(20.0, 20.0, (SRC_HW[1] - 1) * 0.5, (SRC_HW[0] - 1) * 0.5), D=ref.LENSES[lens],
                new_K=(20.0, 20.0, (dst_hw[1] - 1) * 0.5 + shift, (dst_hw[0] - 1) * 0.5))


def small_maps(dst_hw, lens, n_maps):
    if lens == "crafted":
        return [ref.crafted_map(SRC_HW, dst_hw, m) for m in range(n_maps)]
    return [ref.build_map(dst_hw=dst_hw, **small_camera(dst_hw, lens, m)) for m in range(n_maps)]


def uv_independent(K, D, dst_hw):
    """u, v of every destination pixel for new_K = K, R = I in float64, associated differently from the header: the normalised coordinates by
    division, both radial polynomials through np.polyval, the tangential terms expanded."""
    fx, fy, cx, cy = K
    k1, k2, p1, p2, k3, k4, k5, k6 = list(D) + [0.0] * (8 - len(D))
    x, y = np.meshgrid(np.arange(dst_hw[1], dtype=np.float64), np.arange(dst_hw[0], dtype=np.float64))
    xn, yn = (x - cx) / fx, (y - cy) / fy
    r2 = xn ** 2 + yn ** 2
    kr = np.polyval([k3, k2, k1, 1.0], r2) / np.polyval([k6, k5, k4, 1.0], r2)
    xd = xn * kr + 2 * p1 * xn * yn + p2 * r2 + 2 * p2 * xn ** 2
    yd = yn * kr + p1 * r2 + 2 * p1 * yn ** 2 + 2 * p2 * xn * yn
    return fx * xd + cx, fy * yd + cy


def taps_inside(xy, src_hw):
    """per entry: all four taps inside the source, and all four outside"""
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    x_in = [(v >= 0) & (v < src_hw[1]) for v in (sx, sx + 1)]
    y_in = [(v >= 0) & (v < src_hw[0]) for v in (sy, sy + 1)]
    return x_in[0] & x_in[1] & y_in[0] & y_in[1], ~((x_in[0] | x_in[1]) & (y_in[0] | y_in[1]))


@pytest.mark.parametrize("lens", MODEL_LENSES)
def test_built_maps_equal_the_restatement_bit_for_bit(lens):
    for dst_hw, cam in [(MODEL_HW, dict(K=MODEL_K, D=ref.LENSES[lens]))] + [(hw, small_camera(hw, lens, 1)) for hw in DST_HWS]:
        for m, n_maps in ((0, 1), (1, 3)):      # alone, and between two other maps of the tables
            xy, frac = emu.build_map(dst_hw=dst_hw, map=m, n_maps=n_maps, **cam)
            want_xy, want_frac = ref.build_map(dst_hw=dst_hw, **cam)
            assert np.array_equal(xy, want_xy) and np.array_equal(frac, want_frac), (lens, dst_hw)
            assert frac.max() < 1024


def test_rotation_and_rational_terms_equal_the_restatement():
    """a rectifying rotation and a new camera matrix: W is no longer 1"""
    a = 0.05
    R = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    cam = dict(K=MODEL_K, D=ref.LENSES["rational"], new_K=(36.0, 38.0, 30.0, 25.0), R=R)
    xy, frac = emu.build_map(dst_hw=MODEL_HW, **cam)
    want_xy, want_frac = ref.build_map(dst_hw=MODEL_HW, **cam)
    assert np.array_equal(xy, want_xy) and np.array_equal(frac, want_frac)
    assert not np.array_equal(xy, ref.build_map(dst_hw=MODEL_HW, **dict(cam, R=None))[0])


@pytest.mark.parametrize("lens", MODEL_LENSES)
def test_model_against_an_independent_evaluation(lens):
    """Every entry is the rounding of the independently evaluated coordinate: |iu - 32 u| <= 0.5 (rint's half unit) + 1e-6 (fp64 noise)."""
    xy, frac = emu.build_map(dst_hw=MODEL_HW, K=MODEL_K, D=ref.LENSES[lens])
    u, v = uv_independent(MODEL_K, ref.LENSES[lens], MODEL_HW)
    iu = xy[..., 0].astype(np.int64) * 32 + (frac & 31)
    iv = xy[..., 1].astype(np.int64) * 32 + (frac >> 5)
    eu, ev = np.abs(iu - 32 * u).max(), np.abs(iv - 32 * v).max()
    print("%s: max |iu - 32u| %.6f, max |iv - 32v| %.6f" % (lens, eu, ev))
    assert eu <= 0.5 + 1e-6 and ev <= 0.5 + 1e-6
    inside, outside = taps_inside(xy, MODEL_HW)
    x, y = np.meshgrid(np.arange(MODEL_HW[1]), np.arange(MODEL_HW[0]))
    shift = max(np.abs(u - x).max(), np.abs(v - y).max())      # along an axis
    print("%s: inside %.1f %%, wholly outside %.1f %%, displacement up to %.1f px" % (lens, 100 * inside.mean(), 100 * outside.mean(), shift))
    if lens == "pincushion":        # this lens exercises the border
        assert round(100 * inside.mean()) == 81 and round(100 * outside.mean()) == 13
    else:
        assert inside.all() and round(shift, 1) == {"barrel": 4.7, "rational": 7.3}[lens]


def test_ramp_is_reproduced_within_the_physical_bound():
    """The source is the u8 rounding of a ramp a*u + b*v + c.  A destination pixel whose four taps are inside lies within 1 + (|a| + |b|) / 64
    of the ramp at its exact (u, v): the two roundings and the 1/64-pixel coordinate error.  The barrel lens covers every pixel."""
    a, b, c = 2.25, -1.5, 90.0
    xs, ys = np.meshgrid(np.arange(MODEL_HW[1], dtype=np.float64), np.arange(MODEL_HW[0], dtype=np.float64))
    ramp = a * xs + b * ys + c
    assert ramp.min() >= 0 and ramp.max() <= 255
    src = np.repeat(np.rint(ramp).astype(np.uint8)[..., None], 3, -1)
    maps = [emu.build_map(dst_hw=MODEL_HW, K=MODEL_K, D=ref.LENSES["barrel"])]
    got = emu.remap(src[None], maps)[0].astype(np.float64)
    u, v = uv_independent(MODEL_K, ref.LENSES["barrel"], MODEL_HW)
    inside, _ = taps_inside(maps[0][0], MODEL_HW)
    assert inside.mean() == 1.0
    err = np.abs(got - (a * u + b * v + c)[..., None])[inside]
    print("ramp: max error %.4f, bound %.4f" % (err.max(), 1 + (abs(a) + abs(b)) / 64))
    assert err.max() <= 1 + (abs(a) + abs(b)) / 64


def test_identity_and_integer_translation_are_exact():
    img = noise((2,) + MODEL_HW + (3,), 1)
    xy, frac = emu.build_map(dst_hw=MODEL_HW, K=MODEL_K)
    xs, ys = np.meshgrid(np.arange(MODEL_HW[1]), np.arange(MODEL_HW[0]))
    assert np.array_equal(xy[..., 0], xs) and np.array_equal(xy[..., 1], ys) and not frac.any()
    assert np.array_equal(emu.remap(img, [(xy, frac)], n_streams=1), img)
    for tx, ty in ((5, 0), (-3, 2)):        # cx' = cx + tx: destination x reads source x - tx, zeros enter at the edge
        m = emu.build_map(dst_hw=MODEL_HW, K=MODEL_K, new_K=(40.0, 40.0, 31.5 + tx, 23.5 + ty))
        assert not m[1].any()
        want = np.zeros_like(img)
        H, W = MODEL_HW
        want[:, max(ty, 0):H + min(ty, 0), max(tx, 0):W + min(tx, 0)] = img[:, max(-ty, 0):H - max(ty, 0), max(-tx, 0):W - max(tx, 0)]
        assert np.array_equal(emu.remap(img, [m], n_streams=1), want), (tx, ty)
    crop = emu.build_map(dst_hw=(20, 30), K=MODEL_K, new_K=(40.0, 40.0, 31.5 - 10, 23.5 - 8))      # a cropping destination
    assert np.array_equal(emu.remap(img, [crop], n_streams=1), img[:, 8:28, 10:40])


@pytest.mark.parametrize("dst_hw", DST_HWS)
@pytest.mark.parametrize("lens", ("barrel", "pincushion"))
def test_frames_equal_the_restatement_byte_for_byte(dst_hw, lens):
    frames = noise((3,) + SRC_HW + (3,), dst_hw[1])
    maps = small_maps(dst_hw, lens, 2)
    want = ref.remap_batch(frames, maps, [0, 1, 1], 3)
    _, outside = taps_inside(maps[0][0], SRC_HW)
    assert outside.any() and not outside.all()      # the destination is wider than the source: the border is exercised
    for off in (0, 1, 2):
        r = emu.run(frames, maps, dst_offset=off)
        assert not r.staged                             # rows of 87 bytes: the direct form
        assert (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and r.guard_ok, (dst_hw, off, vars(r))
        assert np.array_equal(r.out, want), (dst_hw, off)
        runs = 3 * dst_hw[0] * (dst_hw[1] // 4)
        if dst_hw[1] % 4 == 0:       # every run's entries aligned: all map loads wide, and all stores or none with the pointer
            assert r.wide_loads == 2 * runs and r.wide_stores == (runs if off == 0 else 0)
        else:
            assert 0 < r.wide_loads < 2 * runs and r.wide_stores < runs and (r.wide_stores > 0 or off % 2)


STAGED_SRC_HW = (23, 32)                            # rows of 96 bytes: the staged form's condition


@pytest.mark.parametrize("dst_hw", DST_HWS + ((36, 36),))
@pytest.mark.parametrize("lens", ("barrel", "pincushion", "crafted"))
def test_staged_form_equals_the_restatement_and_the_direct_form(dst_hw, lens):
    """a source whose rows are multiples of 16 bytes at a 16-byte aligned pointer goes through the LDS-staged workgroups: the same bytes as
    the restatement and as the direct form, every staged load inside the frames and aligned; any other pointer takes the direct form"""
    sh, sw = STAGED_SRC_HW
    frames = noise((3, sh, sw, 3), dst_hw[1] + 1)
    frames[:, -1, -3:] = 255
    if lens == "crafted":
        maps = [ref.crafted_map(STAGED_SRC_HW, dst_hw, m) for m in range(2)]
    else:
        maps = [ref.build_map((20.0, 20.0, (sw - 1) * 0.5, (sh - 1) * 0.5), ref.LENSES[lens], (20.0, 20.0, (dst_hw[1] - 1) * 0.5 + m, (dst_hw[0] - 1) * 0.5),
                              dst_hw=dst_hw) for m in range(2)]
    want = ref.remap_batch(frames, maps, [0, 1, 1], 3)
    for off in (0, 1):
        r = emu.run(frames, maps, dst_offset=off)
        assert r.staged and r.staged_loads > 0 and r.direct_tiles == 0
        assert (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and r.guard_ok, (dst_hw, lens, off, vars(r))
        assert np.array_equal(r.out, want), (dst_hw, lens, off)
    for kw in (dict(path=0), dict(src_offset=16), dict(src_offset=4)):
        r = emu.run(frames, maps, **kw)
        assert r.staged == (kw == dict(src_offset=16)) and (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and np.array_equal(r.out, want), kw


@pytest.mark.parametrize("lens", MODEL_LENSES)
def test_staged_form_at_the_model_size(lens):
    frames = noise((2,) + MODEL_HW + (3,), 9)
    maps = [ref.build_map(MODEL_K, ref.LENSES[lens], dst_hw=MODEL_HW)]
    r = emu.run(frames, maps, n_streams=1)
    assert r.staged and r.direct_tiles == 0 and (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and r.guard_ok
    assert np.array_equal(r.out, ref.remap_batch(frames, maps, [0], 1))


def test_staged_form_gathers_directly_where_the_box_does_not_fit():
    """a 2048x12 source (6144 bytes a row) under the crafted map: a workgroup's taps span the whole frame, 72 KB against the 16 KB of LDS, so
    it takes the direct form's gathers; a second map that stays in one corner is staged by the same launch"""
    src_hw, dst_hw = (12, 2048), (8, 300)
    frames = noise((2,) + src_hw + (3,), 13)
    wide = ref.crafted_map(src_hw, dst_hw)
    xs, ys = np.meshgrid(np.arange(dst_hw[1]) % 40, np.arange(dst_hw[0]))
    corner = (np.stack([xs, ys], -1).astype(np.int16), np.full(dst_hw, 5 * 32 + 7, np.uint16))
    r = emu.run(frames, [wide, corner], n_streams=2)
    assert r.staged and r.direct_tiles == 2 * 2 and r.staged_loads > 0     # frame 0: two tile rows by two tile columns, none fits
    assert (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and r.guard_ok
    assert np.array_equal(r.out, ref.remap_batch(frames, [wide, corner], [0, 1], 2))


def test_crafted_map_hits_every_branch_of_the_sampler():
    """36x36 over the 29x23 source: sx, sy out of {-32768, -2, -1, 0, n-3, n-2, n-1, n, 32767} and fractions out of {0, 1, 16, 31}, every
    combination once: the 8-byte fast path up to its last legal column n-3, every partial case, the wholly outside and the saturated entries."""
    xy, frac = ref.crafted_map(SRC_HW, (36, 36))
    combos = set(zip(xy[..., 0].ravel().tolist(), xy[..., 1].ravel().tolist(), (frac & 31).ravel().tolist(), ((frac >> 5) & 31).ravel().tolist()))
    assert len(combos) == 9 * 9 * 4 * 4 == 36 * 36 and (frac >> 10).any()
    sx, sy = xy[..., 0].astype(int), xy[..., 1].astype(int)
    fast = (sx >= 0) & (sy >= 0) & (sy + 1 < SRC_HW[0]) & (sx * 3 + 8 <= SRC_HW[1] * 3)
    inside, outside = taps_inside(xy, SRC_HW)
    assert fast.any() and (fast & (sx == SRC_HW[1] - 3)).any() and not (fast & (sx == SRC_HW[1] - 2)).any()
    assert (inside & ~fast).any() and outside.any() and (~inside & ~outside).any()
    frames = noise((2,) + SRC_HW + (3,), 7)
    frames[:, -1, -3:] = 255                      # the last bytes of a frame under full weight
    for off in (0, 3):
        r = emu.run(frames, [(xy, frac)], n_streams=1, dst_offset=off)
        assert (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and r.guard_ok
        assert np.array_equal(r.out, ref.remap_batch(frames, [(xy, frac)], [0], 1))
    assert np.array_equal(ref.remap(frames[0], xy, frac), ref.remap(frames[0], xy, frac & 1023))      # U1: the top 6 bits are ignored


def test_every_frame_uses_its_streams_map():
    """U5: 3 streams, 2 maps, micro-batch 2: frame f = b * 3 + s reads the map of stream s"""
    dst_hw = DST_HWS[1]
    frames = noise((6,) + SRC_HW + (3,), 3)
    maps = small_maps(dst_hw, "barrel", 2)
    assert emu.default_stream_map(3, 2) == [0, 1, 1] and emu.default_stream_map(4, 1) == [0, 0, 0, 0] and emu.default_stream_map(2, 3) == [0, 1]
    for table in (None, [1, 0, 1], [0, 0, 0]):
        got = emu.remap(frames, maps, table, 3)
        sm = [0, 1, 1] if table is None else table
        for f in range(6):
            assert np.array_equal(got[f], ref.remap(frames[f], *maps[sm[f % 3]])), (table, f)
            assert not np.array_equal(got[f], ref.remap(frames[f], *maps[1 - sm[f % 3]]))      # the other map would have shown


def test_refusals_by_number_and_name():
    """U4 through the header"""
    assert [emu.why(k) for k in range(1, 6)] == [emu.WHY[k] for k in range(1, 6)] and emu.why(0) == ""
    K, ok = MODEL_K, dict(K=MODEL_K, D=ref.LENSES["rational"])
    assert emu.check_camera(**ok) is None
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert emu.check_camera((bad,) + K[1:]) == "non-finite parameter"
        assert emu.check_camera(K, (0, 0, 0, 0, 0, 0, 0, bad)) == "non-finite parameter"
        assert emu.check_camera(K, new_K=K[:3] + (bad,)) == "non-finite parameter"
        assert emu.check_camera(K, R=[1, 0, 0, 0, 1, 0, 0, bad, 1]) == "non-finite parameter"
    for i in (0, 1):
        z = tuple(0.0 if j == i else v for j, v in enumerate(K))
        assert emu.check_camera(z) == "zero focal length" and emu.check_camera(K, new_K=z) == "zero focal length"
    assert emu.check_camera(K, R=[1, 0, 0, 0, 1, 0, 0, 0, 0]) == "singular new_K * R"
    assert emu.check_camera(K, R=[1, 2, 3, 2, 4, 6, 0, 0, 1]) == "singular new_K * R"
    size = emu.WHY[4]
    assert emu.check_sizes((4320, 16384), (4320, 16384)) is None and emu.check_sizes((1, 1), (1, 1)) is None
    assert emu.check_sizes((4321, 8), (8, 8)) == size and emu.check_sizes((8, 16385), (8, 8)) == size
    assert emu.check_sizes((8, 8), (0, 8)) == size and emu.check_sizes((8, 8), (8, 16385)) == size and emu.check_sizes((8, 0), (8, 8)) == size
    assert emu.check_map(0, 1) is None and emu.check_map(1, 1) == emu.WHY[5] and emu.check_map(-1, 2) == emu.WHY[5]
    assert [emu.map_stride(hw) for hw in DST_HWS] == [900, 928, 952, 976]


def test_layouts_three_ways(tmp_path):
    """adas_remap_params and adas_remap_camera as gcc compiles the public header, _lib's mirrors, the emulation's view (g++ on the public header,
    the core header's RemapCamera) and its ctypes mirrors"""
    load_pkg()
    L = importlib.import_module("adas_amd._lib")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "adas_hip.h"', 'int main(void) {',
             '  printf("psize %zu\\n", sizeof(adas_remap_params));', '  printf("csize %zu\\n", sizeof(adas_remap_camera));']
    for fname in emu.PARAM_FIELDS:
        lines.append('  printf("p.%s %%zu\\n", offsetof(adas_remap_params, %s));' % (fname, fname))
    for fname in emu.CAMERA_FIELDS:
        lines.append('  printf("c.%s %%zu\\n", offsetof(adas_remap_camera, %s));' % (fname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split(" ", 1) for l in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    (psize, poff), (csize, coff) = emu.layout()
    assert int(got["psize"]) == C.sizeof(L.RemapParams) == C.sizeof(emu.Params) == psize == 24
    assert int(got["csize"]) == C.sizeof(L.RemapCamera) == C.sizeof(emu.Camera) == csize == 25 * 8
    assert tuple(f for f, _ in L.RemapParams._fields_) == tuple(f for f, _ in emu.Params._fields_) == emu.PARAM_FIELDS
    assert tuple(f for f, _ in L.RemapCamera._fields_) == tuple(f for f, _ in emu.Camera._fields_) == emu.CAMERA_FIELDS
    for f in emu.PARAM_FIELDS:
        assert int(got["p." + f]) == getattr(L.RemapParams, f).offset == getattr(emu.Params, f).offset == poff[f], f
    for f in emu.CAMERA_FIELDS:
        assert int(got["c." + f]) == getattr(L.RemapCamera, f).offset == getattr(emu.Camera, f).offset == coff[f], f


def test_refusals_arrive_by_name_through_create_and_set_camera():
    """adas_remap_create and adas_remap_set_camera check their arguments before they touch a device"""
    load_pkg()
    L = importlib.import_module("adas_amd._lib")

    def create(src_hw=(23, 29), dst_hw=(25, 37), n_streams=3, n_maps=2, max_batch=6):
        p = L.RemapParams(src_hw[0], src_hw[1], dst_hw[0], dst_hw[1], n_streams, n_maps)
        h_ = C.c_void_p()
        L.check(L.lib().adas_remap_create(C.byref(p), max_batch, C.byref(h_)))
        return h_

    for kw, match in ((dict(src_hw=(4321, 29)), "adas_remap_create: size outside 1..4320 rows x 1..16384 columns"),
                      (dict(dst_hw=(25, 0)), "adas_remap_create: size outside"), (dict(dst_hw=(25, 16385)), "adas_remap_create: size outside"),
                      (dict(n_streams=0), "adas_remap_create: n_streams 0"), (dict(n_maps=0), "adas_remap_create: n_maps 0"),
                      (dict(max_batch=0), "adas_remap_create: max_batch 0")):
        with pytest.raises(RuntimeError, match=match) as ei:
            create(**kw)
        assert ei.value.code == -1
    h_ = create()
    try:
        def cam(**kw):
            c = emu.camera(**dict(dict(K=MODEL_K, D=ref.LENSES["barrel"]), **kw))
            return C.cast(C.pointer(c), C.POINTER(L.RemapCamera))

        for m, kw, match in ((0, dict(K=(float("nan"), 40, 31.5, 23.5)), "adas_remap_set_camera: non-finite parameter"),
                             (0, dict(D=(0, 0, float("inf"), 0)), "adas_remap_set_camera: non-finite parameter"),
                             (0, dict(K=(40, 0, 31.5, 23.5)), "adas_remap_set_camera: zero focal length"),
                             (0, dict(new_K=(0, 40, 31.5, 23.5)), "adas_remap_set_camera: zero focal length"),
                             (-1, dict(R=[1, 0, 0, 0, 1, 0, 0, 0, 0]), "adas_remap_set_camera: singular new_K \\* R"),
                             (2, {}, "adas_remap_set_camera: map index outside the handle's table \\(map 2 of 2\\)"),
                             (-2, {}, "adas_remap_set_camera: map index outside the handle's table")):
            with pytest.raises(RuntimeError, match=match) as ei:
                L.check(L.lib().adas_remap_set_camera(h_, m, cam(**kw)))
            assert ei.value.code == -1
        xy, frac = ref.crafted_map((23, 29), (25, 37))
        for fn, args in ((L.lib().adas_remap_set_map, (2, L.ptr(xy), L.ptr(frac))), (L.lib().adas_remap_fetch_map, (-1, L.ptr(xy), L.ptr(frac))),
                         (L.lib().adas_remap_assign, (0, 2))):
            with pytest.raises(RuntimeError, match="map index outside the handle's table"):
                L.check(fn(h_, *args))
        with pytest.raises(RuntimeError, match="adas_remap_assign: stream 3 of 3"):
            L.check(L.lib().adas_remap_assign(h_, 3, 0))
        L.check(L.lib().adas_remap_assign(h_, 2, 0))
    finally:
        L.lib().adas_remap_destroy(h_)


def test_pipeline_arguments_without_a_gpu():
    """AdasPipeline(undistort=...) and FrameRemapper refuse by ValueError naming the key, before any engine or handle is created."""
    load_pkg()
    PL = importlib.import_module("adas_amd.pipeline")
    PP = importlib.import_module("adas_amd.postproc")
    missing = "/nonexistent/model.hipm"          # never opened: every check below comes first
    K, D = (1000.0, 1000.0, 639.5, 359.5), (-0.3, 0.1, 0.0, 0.0)
    xy, frac = np.zeros((720, 1280, 2), np.int16), np.zeros((720, 1280), np.uint16)
    for kw, match in ((dict(camera=dict(K=K, D=D), lens="wide"), "undistort= holds unknown keys \\['lens'\\]"),
                      ({}, "undistort= needs exactly one of camera=, cameras= and maps="),
                      (dict(camera=dict(K=K), maps=[(xy, frac)]), "undistort= needs exactly one of"),
                      (dict(camera=dict(K=K, D=D, alpha=0)), "undistort= camera holds unknown keys \\['alpha'\\]"),
                      (dict(camera=dict(D=D)), "undistort= camera needs K"),
                      (dict(camera=dict(K=K[:3], D=D)), "undistort= camera K .* has the wrong shape"),
                      (dict(camera=dict(K=K, D=D[:3])), "undistort= camera D .* has the wrong shape"),
                      (dict(camera=dict(K=K, D=D, R=(1, 0, 0, 1))), "undistort= camera R .* has the wrong shape"),
                      (dict(camera=dict(K=K, D=(float("nan"), 0, 0, 0))), "undistort= camera D .* holds a non-finite parameter"),
                      (dict(camera=[K, D]), "undistort= camera .* is no dict"),
                      (dict(cameras=[dict(K=K, D=D)]), "undistort= cameras holds 1 cameras, the pipeline has 2 streams"),
                      (dict(cameras=[dict(K=K, D=D), dict(K=K, D=D, new_K=(1, 2))]), "undistort= cameras\\[1\\] camera new_K .* has the wrong shape"),
                      (dict(cameras=[dict(K=K)] * 2, stream_map=[0, 0]), "undistort= stream_map goes with maps="),
                      (dict(maps=[(xy, frac), xy]), "undistort= maps .* is no list of \\(xy, frac\\) pairs"),
                      (dict(maps=[(xy.astype(np.float32), frac)]), "undistort= maps\\[0\\] xy is float32"),
                      (dict(maps=[(xy[:, :-1], frac)]), "undistort= maps\\[0\\] xy is int16 \\(720, 1279, 2\\), not int16 \\(720, 1280, 2\\)"),
                      (dict(maps=[(xy, frac.astype(np.int16))]), "undistort= maps\\[0\\] frac is int16"),
                      (dict(maps=[(xy, frac)], stream_map=[0]), "undistort= stream_map \\[0\\] is no list of 2 map indices"),
                      (dict(maps=[(xy, frac)], stream_map=[0, 1]), "undistort= stream_map\\[1\\] = 1 is outside the 1 maps")):
        with pytest.raises(ValueError, match=match):
            PL.AdasPipeline(None, missing, n_streams=2, undistort=kw)
    with pytest.raises(ValueError, match="undistort= 'barrel' is neither None nor a dict"):
        PL.AdasPipeline(None, missing, undistort="barrel")
    a = PP.undistort_args(dict(cameras=[dict(K=K, D=D), dict(K=K, D=D[:2] + (0.001, 0)), dict(K=np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]),
                                                                                          D=D + (0.0,))]), 3, (720, 1280))
    assert a["stream_map"] == [0, 1, 0] and len(a["cameras"]) == 2      # identical cameras share one map, however they were written
    assert a["cameras"][0] == dict(K=K, D=D + (0.0,) * 4, new_K=K, R=(1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0))
    assert PP.undistort_args(dict(maps=[(xy, frac)] * 2), 3, (720, 1280))["stream_map"] == [0, 1, 1]
    for kw, match in ((dict(cameras=[dict(K=K)], maps=[(xy, frac)]), "needs cameras= or maps=, not both"), ({}, "needs cameras= or maps=, not both"),
                      (dict(cameras=[]), "at least one camera or map"), (dict(cameras=[dict(K=K)], stream_map=[0, 1]), "stream_map\\[1\\] = 1 is outside")):
        with pytest.raises(ValueError, match=match):
            PP.FrameRemapper((720, 1280), 2, **kw)


def test_for_rank_takes_its_own_streams_cameras():
    """a job-wide cameras= or stream_map= list is dealt to the ranks as the streams are (stream s -> rank s mod world): rank 1 of 2 holds
    streams 1 and 3, so the bad entry 3 of the job is its local entry 1, and rank 0 does not see it"""
    load_pkg()
    PL = importlib.import_module("adas_amd.pipeline")
    SH = importlib.import_module("adas_amd.sharding")
    missing = "/nonexistent/model.hipm"
    K = (1000.0, 1000.0, 639.5, 359.5)
    cams = [dict(K=K), dict(K=K), dict(K=K), dict(K=K[:3])]
    with pytest.raises(ValueError, match="undistort= cameras\\[1\\] camera K .* has the wrong shape"):
        PL.AdasPipeline.for_rank(None, missing, 4, env=SH.RankEnv(1, 1, 2), undistort=dict(cameras=cams))
    with pytest.raises(Exception) as ei:        # rank 0's cameras are fine: it gets as far as the model file
        PL.AdasPipeline.for_rank(None, missing, 4, env=SH.RankEnv(0, 0, 2), undistort=dict(cameras=cams))
    assert not isinstance(ei.value, ValueError) or "undistort" not in str(ei.value)
    xy, frac = np.zeros((720, 1280, 2), np.int16), np.zeros((720, 1280), np.uint16)
    with pytest.raises(ValueError, match="undistort= stream_map\\[1\\] = 5 is outside the 1 maps"):
        PL.AdasPipeline.for_rank(None, missing, 4, env=SH.RankEnv(1, 1, 2), undistort=dict(maps=[(xy, frac)], stream_map=[0, 0, 0, 5]))


def test_bounds_program_under_the_sanitizers():
    """tests/hostemu/remap_bounds_main.cpp with -fsanitize=address,undefined, its own main, run as a child process: both kernels' work items
    over heap blocks that end exactly where the frames, the maps and the table end; the checksums are the restatement's.  The sanitizers'
    runtimes are linked statically, so the program runs in whatever environment the suite has."""
    exe = os.path.join(emu.ROOT, "tests", "_build", "remap_bounds")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", emu.INC, "-I", emu.PUB, emu.MAIN, "-o", exe])
    # src_w, src_h, dst_w, dst_h, n_streams, n_maps, batch, lens, align
    names = ("identity", "barrel", "rational", "pincushion", "crafted")
    cases = [(29, 23, dw, 25, 3, 2, 6, lens, align) for dw in (36, 37, 38, 39) for lens, align in ((1, 0), (3, 1), (4, 2))]
    cases += [(29, 23, 36, 36, 1, 1, 2, 4, 0), (29, 23, 36, 36, 1, 1, 2, 4, 3), (64, 48, 64, 48, 1, 1, 1, 2, 0), (64, 48, 64, 48, 2, 2, 3, 3, 5),
              (29, 23, 29, 23, 2, 1, 3, 0, 0), (1, 1, 5, 3, 1, 1, 1, 0, 1), (2, 2, 9, 1, 1, 1, 2, 4, 0)]
    # rows that are multiples of 16 bytes: the staged form (malloc's blocks are 16-byte aligned), also where its boxes do not fit
    cases += [(32, 23, dw, 25, 3, 2, 6, lens, 0) for dw in (36, 37, 38, 39) for lens in (1, 3, 4)]
    cases += [(32, 23, 36, 36, 1, 1, 2, 4, 0), (16, 3, 300, 5, 1, 1, 2, 4, 0), (2048, 12, 300, 8, 1, 1, 2, 4, 0), (32, 23, 37, 25, 3, 2, 6, 4, 4)]
    p = subprocess.run([exe] + [",".join(str(v) for v in c) for c in cases], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        sw, sh, dw, dh, n_streams, n_maps, batch, lens, align = c
        frames = ref.lcg_bytes(batch * sh * sw * 3).reshape(batch, sh, sw, 3)
        if lens == 4:
            maps = [ref.crafted_map((sh, sw), (dh, dw), m) for m in range(n_maps)]
        else:
            maps = [ref.build_map((20.0, 20.0, (sw - 1) * 0.5, (sh - 1) * 0.5), ref.LENSES[names[lens]], (20.0, 20.0, (dw - 1) * 0.5 + m, (dh - 1) * 0.5),
                                  dst_hw=(dh, dw)) for m in range(n_maps)]
        want = ref.remap_batch(frames, maps, emu.default_stream_map(n_streams, n_maps), n_streams)
        s = 2166136261
        for b in want.tobytes():
            s = ((s ^ b) * 16777619) & 0xFFFFFFFF
        staged = int((sw * 3) % 16 == 0 and align == 0)
        assert line == "%s %08x staged %d outside 0 misaligned 0 not_once 0 build_bad 0" % (",".join(str(v) for v in c), s, staged), (c, line)
