"""CPU: the bird-view image warp (cv2.warpPerspective, 8-bit INTER_LINEAR, BORDER_CONSTANT 0).
  1. invariants of the NumPy restatement (tests/warp_ref.py; parity with a real cv2 build is unpinned);
  2. the restatement against an independent float64 bilinear (torch grid_sample fed the exact projective coordinates);
  3. the host build of csrc/warp_core.h -- the text the device kernel runs -- against the restatement, every byte;
  4. adas_warp_params against its ctypes mirror, and the singular-matrix error of adas_warp_set_matrix (host state only)."""
import ctypes as C
import importlib, os, subprocess

import numpy as np
import pytest

from conftest import load_pkg, ROOT
import warp_ref

load_pkg()
A = importlib.import_module("adas_amd.analysis")


def view_matrices(w, h):
    pt = A.PerspectiveTransformation((w, h))
    return pt.M, pt.M_inv


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def warp_cases():
    """(name, source image, matrix, dst (w, h), inverse flag): the shapes at which the kernel's paths differ -- three 64-pixel blocks
    with dst_w % 4 == 3, widths 1 and 5 (one run, tail only / one full run + tail), a frontal matrix whose W passes through 0 inside
    the destination (coordinates run off to the int32 clamp next to it), tap columns past the 16-bit saturation."""
    src = noise(45, 70, 11)
    M, M_inv = view_matrices(131, 37)
    T = np.array([[1.0, 0, 7], [0, 1, -4], [0, 0, 1]])
    big = M @ np.diag([1 / 3.0e3, 1 / 3.0e3, 1.0])             # source coordinates x3000: most tap columns leave int16
    return [
        ("bird", src, M, (131, 37), False),
        ("frontal", src, M_inv, (131, 37), False),
        ("translate", src, T, (131, 37), False),
        ("saturate", src, big, (131, 37), False),
        ("inverse_flag", src, M_inv, (131, 37), True),
        ("w1", src, M, (1, 37), False),
        ("w5", src, M_inv, (5, 37), False),
        ("identity64", noise(64, 64, 12), np.eye(3), (64, 64), False),
    ]


# ---------------------------------------------------------------------------------------------- 1. restatement invariants
def test_restatement_identity_and_translation():
    img = noise(45, 70, 1)
    np.testing.assert_array_equal(warp_ref.warp_perspective(img, np.eye(3), (70, 45)), img)
    for tx, ty in ((7, -4), (-13, 9), (0, 44), (69, 0)):
        T = np.array([[1.0, 0, tx], [0, 1, ty], [0, 0, 1]])
        want = np.zeros_like(img)
        ys, xs = np.mgrid[0:45, 0:70]
        ok = (ys - ty >= 0) & (ys - ty < 45) & (xs - tx >= 0) & (xs - tx < 70)
        want[ok] = img[(ys - ty)[ok], (xs - tx)[ok]]
        np.testing.assert_array_equal(warp_ref.warp_perspective(img, T, (70, 45)), want)
    assert (warp_ref.warp_perspective(img, np.array([[1.0, 0, 70], [0, 1, 0], [0, 0, 1]]), (70, 45)) == 0).all()


def test_restatement_inverse_flag_and_singular():
    img = noise(45, 70, 2)
    M, _ = view_matrices(131, 37)
    a = warp_ref.warp_perspective(img, M, (131, 37))
    b = warp_ref.warp_perspective(img, warp_ref.invert3x3(M), (131, 37), inverse=True)
    np.testing.assert_array_equal(a, b)
    assert a.any()
    np.testing.assert_allclose(warp_ref.invert3x3(M).reshape(3, 3) @ M, np.eye(3), atol=1e-9)
    with pytest.raises(ValueError):
        warp_ref.invert3x3(np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]))
    assert warp_ref.block_width(720, 1280) == 64 and warp_ref.block_width(37, 131) == 64
    assert warp_ref.block_width(37, 5) == 5 and warp_ref.block_width(8, 1280) == 128


# ---------------------------------------------------------------------------------------------- 2. vs an independent float bilinear
@pytest.mark.parametrize("w,h", [(131, 37), (160, 96)])
def test_restatement_vs_float_bilinear(w, h):
    """On pixels whose exact source point lies at least one pixel inside the frame, |restatement - float64 bilinear| <=
    0.5 + (gx + gy)/64 + 1e-6: the coordinate is quantised to 1/32 px (off by at most 1/64 px per axis) on a surface that is
    Lipschitz with the adjacent-pixel differences gx, gy; the weights are exact, so the shift costs one rounding of 0.5."""
    import torch
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([40 + 1.1 * xs + 0.6 * ys, 128 + 60 * np.sin(xs / 17.0) * np.cos(ys / 11.0), 250 - 0.9 * xs - 1.2 * ys], -1)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    f = img.astype(np.float64)
    gx = np.abs(np.diff(f, axis=1)).max()
    gy = np.abs(np.diff(f, axis=0)).max()
    assert 0 < gx <= 8 and 0 < gy <= 8                                     # smooth by construction
    bound = 0.5 + (gx + gy) / 64 + 1e-6
    t = torch.from_numpy(f).permute(2, 0, 1)[None]
    for M, keep in zip(view_matrices(w, h), (0.60, 0.20)):
        Mi = np.linalg.inv(M)
        q = np.einsum("kl,hwl->hwk", Mi, np.stack([xs, ys, np.ones_like(xs)], -1))
        with np.errstate(all="ignore"):
            u, v = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
        mask = np.isfinite(u) & np.isfinite(v) & (u >= 1) & (u <= w - 2) & (v >= 1) & (v <= h - 2)
        assert mask.mean() >= keep, mask.mean()
        grid = np.stack([2 * u / (w - 1) - 1, 2 * v / (h - 1) - 1], -1)
        grid = np.where(mask[..., None], grid, -5.0)
        want = torch.nn.functional.grid_sample(t, torch.from_numpy(grid)[None], mode="bilinear", padding_mode="zeros", align_corners=True)
        want = want[0].permute(1, 2, 0).numpy()
        got = warp_ref.warp_perspective(img, M, (w, h)).astype(np.float64)
        err = np.abs(got - want)[mask]
        print("float bilinear %dx%d keep %.2f: max err %.4f, bound %.4f" % (w, h, mask.mean(), err.max(), bound))
        assert err.max() <= bound, (err.max(), bound)


# ---------------------------------------------------------------------------------------------- 3. host build of warp_core.h
@pytest.mark.parametrize("case", warp_cases(), ids=lambda c: c[0])
def test_host_build_equals_restatement(case):
    import emu_warp_api
    name, src, M, dst_wh, inverse = case
    want = warp_ref.warp_perspective(src, M, dst_wh, inverse)
    got = emu_warp_api.warp_perspective(src, M, dst_wh, inverse)
    assert got is not None and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    sx, sy, ax, ay = warp_ref.coords(M, (dst_wh[1], dst_wh[0]), inverse)
    if name == "saturate":       # the case is there for the clamps: they must be hit
        assert (sx == 32767).any() and (sy == 32767).any() and (sx < 32767).any()
    if name in ("frontal", "w5"):  # W changes sign inside the destination
        q = np.einsum("kl,hwl->hwk", warp_ref.invert3x3(M).reshape(3, 3),
                      np.stack(list(np.mgrid[0:dst_wh[1], 0:dst_wh[0]][::-1].astype(np.float64)) + [np.ones((dst_wh[1], dst_wh[0]))], -1))
        assert (q[..., 2] > 0).any() and (q[..., 2] < 0).any()
    if name in ("bird", "translate", "identity64"):
        assert want.any()


def test_host_build_inversion_and_blocks():
    import emu_warp_api
    for M in view_matrices(131, 37) + view_matrices(1280, 720):
        np.testing.assert_array_equal(emu_warp_api.invert3x3(M), warp_ref.invert3x3(M))
    sing = np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])
    assert emu_warp_api.invert3x3(sing) is None
    assert emu_warp_api.warp_perspective(noise(4, 4, 0), sing, (4, 4)) is None
    for dh, dw in ((720, 1280), (37, 131), (37, 5), (37, 1), (8, 1280), (1, 2000)):
        assert emu_warp_api.block_width(dh, dw) == warp_ref.block_width(dh, dw)


# ---------------------------------------------------------------------------------------------- 4. ABI
def test_warp_params_layout_and_singular_matrix(tmp_path):
    L = importlib.import_module("adas_amd._lib")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "adas_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(adas_warp_params));']
    for fname, _ in L.WarpParams._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(adas_warp_params, %s));' % (fname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(got["size"]) == C.sizeof(L.WarpParams)
    for fname, _ in L.WarpParams._fields_:
        assert int(got[fname]) == getattr(L.WarpParams, fname).offset, fname
    # the handle and its matrices are host state: no device needed up to the first run
    lib = L.lib()
    h = C.c_void_p()
    p = L.WarpParams(45, 70, 37, 131)
    assert lib.adas_warp_create(C.byref(p), 2, C.byref(h)) == 0
    try:
        sing = np.array([1.0, 2, 3, 2, 4, 6, 0, 0, 1])
        assert lib.adas_warp_set_matrix(h, -1, L.ptr(sing), 0) == -1            # ADAS_ERR_INVALID
        assert b"singular" in lib.adas_last_error()
        assert lib.adas_warp_set_matrix(h, 0, L.ptr(sing), 1) == 0              # used as given with the inverse-map flag
        assert lib.adas_warp_set_matrix(h, 1, L.ptr(np.eye(3).reshape(9)), 0) == 0
        assert lib.adas_warp_set_matrix(h, 2, L.ptr(np.eye(3).reshape(9)), 0) == -1   # frame outside the batch
    finally:
        lib.adas_warp_destroy(h)
    for bad in (L.WarpParams(0, 70, 37, 131), L.WarpParams(45, 70, 37, 16385), L.WarpParams(4321, 70, 37, 131)):
        assert lib.adas_warp_create(C.byref(bad), 1, C.byref(h)) == -1
