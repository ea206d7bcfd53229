"""GPU: warp_perspective_kernel (csrc/warp_kernels.hip) through the C ABI, postproc.PerspectiveWarp and
PerspectiveTransformation.transformToBirdView / transformToFrontalView against the NumPy restatement (tests/warp_ref.py), every byte."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import warp_ref

pytestmark = pytest.mark.gpu
load_pkg()
A = importlib.import_module("adas_amd.analysis")
GUARD = 64      # bytes of 0xA5 on either side of a caller's destination: nothing may be written outside the frames


@pytest.fixture(scope="module")
def G():
    L = importlib.import_module("adas_amd._lib")
    assert L.lib().adas_device_count() > 0, "no HIP device"
    return L, importlib.import_module("adas_amd.postproc"), importlib.import_module("adas_amd.detectors")


def noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def view_matrices(w, h):
    pt = A.PerspectiveTransformation((w, h))
    return pt.M, pt.M_inv


def small_matrices():
    M, M_inv = view_matrices(131, 37)
    T = np.array([[1.0, 0, 7], [0, 1, -4], [0, 0, 1]])
    big = M @ np.diag([1 / 3.0e3, 1 / 3.0e3, 1.0])      # source coordinates x3000: most tap columns saturate at int16
    return M, M_inv, T, big


def run_batch(G, src, mats, dst_wh, inverse=(), offset=16):
    """One launch over len(src) frames, frame f with mats[f] -> (result in a caller's buffer, result in the handle's buffer)."""
    L, PP, _ = G
    n, sh, sw = src.shape[:3]
    dw, dh = dst_wh
    w = PP.PerspectiveWarp((sh, sw), (dh, dw), n)
    sbuf = L.DeviceBuffer.from_array(src)
    nbytes = n * dh * dw * 3
    canvas = np.full(nbytes + 2 * GUARD, 0xA5, np.uint8)
    dbuf = L.DeviceBuffer.from_array(canvas)
    try:
        for f, M in enumerate(mats):
            w.set_matrix(M, f, inverse=f in inverse)
        w.run(sbuf.ptr, n, dbuf.ptr + offset)
        L.check(L.lib().adas_synchronize())
        back = dbuf.download(canvas.shape, np.uint8)
        assert (back[:offset] == 0xA5).all() and (back[offset + nbytes:] == 0xA5).all(), "write outside the destination"
        mine = back[offset:offset + nbytes].reshape(n, dh, dw, 3)
        w.run(sbuf.ptr, n)
        own = np.stack([w.fetch(f) for f in range(n)])
        raw = np.empty_like(own)                                # the same buffer through its device view
        L.check(L.lib().adas_memcpy_d2h(L.ptr(raw), w.device_view(), raw.nbytes))
        assert np.array_equal(raw, own)
        return mine, own
    finally:
        w.close(); sbuf.free(); dbuf.free()


@pytest.mark.parametrize("name,dst_wh,pick,inverse", [
    ("bird_frontal_translate", (131, 37), (0, 1, 2), ()),
    ("saturate_inverseflag_bird", (131, 37), (3, 1, 0), (1,)),
    ("w1", (1, 37), (0, 1, 2), ()),
    ("w5", (5, 37), (1, 0, 3), ()),
])
@pytest.mark.parametrize("offset", [16, 3], ids=["aligned", "odd_base"])
def test_kernel_equals_restatement_small(G, name, dst_wh, pick, inverse, offset):
    """src 45x70 -> dst 37x131 (three 64-pixel blocks, dst_w % 4 == 3: rows start on every byte alignment), widths 1 and 5; one
    batch = 3 launch with three different matrices and three different frames."""
    src = noise(3, 45, 70, 21)
    mats = [small_matrices()[i] for i in pick]
    mine, own = run_batch(G, src, mats, dst_wh, inverse, offset)
    for f in range(3):
        want = warp_ref.warp_perspective(src[f], mats[f], dst_wh, inverse=f in inverse)
        np.testing.assert_array_equal(mine[f], want)
        np.testing.assert_array_equal(own[f], want)


def test_kernel_identity_64(G):
    src = noise(1, 64, 64, 22)
    mine, own = run_batch(G, src, [np.eye(3)], (64, 64))
    np.testing.assert_array_equal(mine[0], src[0])
    np.testing.assert_array_equal(own[0], src[0])


def test_kernel_equals_restatement_720p(G):
    src = noise(2, 720, 1280, 23)
    mats = list(view_matrices(1280, 720))
    mine, own = run_batch(G, src, mats, (1280, 720))
    for f in range(2):
        want = warp_ref.warp_perspective(src[f], mats[f], (1280, 720))
        assert want.any()
        np.testing.assert_array_equal(mine[f], want)
        np.testing.assert_array_equal(own[f], want)


def test_matrix_change_between_runs_and_batch_position(G):
    L, PP, _ = G
    M, M_inv, T, big = small_matrices()
    src = noise(3, 45, 70, 24)
    src[2] = src[0]                                      # the same frame at positions 0 and 2
    w = PP.PerspectiveWarp((45, 70), (37, 131), 3)
    sbuf = L.DeviceBuffer.from_array(src)
    try:
        w.set_matrix(M)                                  # frame = -1: every frame
        w.set_matrix(M_inv, 1)
        w.run(sbuf.ptr, 3)
        a = [w.fetch(f) for f in range(3)]
        np.testing.assert_array_equal(a[0], warp_ref.warp_perspective(src[0], M, (131, 37)))
        np.testing.assert_array_equal(a[1], warp_ref.warp_perspective(src[1], M_inv, (131, 37)))
        np.testing.assert_array_equal(a[2], a[0])        # position in the batch does not matter
        w.set_matrix(T, 1)                               # same handle, one row of the table changes
        w.run(sbuf.ptr, 3)
        b = [w.fetch(f) for f in range(3)]
        np.testing.assert_array_equal(b[1], warp_ref.warp_perspective(src[1], T, (131, 37)))
        assert not np.array_equal(b[1], a[1])
        np.testing.assert_array_equal(b[0], a[0])
        np.testing.assert_array_equal(b[2], a[2])
        w.run(sbuf.ptr, 1)                               # a shorter batch leaves the other frames of the buffer alone
        np.testing.assert_array_equal(w.fetch(1), b[1])
    finally:
        w.close(); sbuf.free()


def test_perspective_transformation_methods(G):
    L, PP, D = G
    img = noise(1, 45, 70, 25)[0]
    pt = A.PerspectiveTransformation((131, 37))
    sbuf = L.DeviceBuffer.from_array(img)
    try:
        staged = D.StagedFrame(sbuf.ptr, 45, 70, 1)
        want = warp_ref.warp_perspective(img, pt.M, (131, 37))
        got = pt.transformToBirdView(img)
        assert got.shape == (37, 131, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(pt.transformToBirdView(staged), want)
        np.testing.assert_array_equal(pt.transformToFrontalView(img), warp_ref.warp_perspective(img, pt.M_inv, (131, 37)))
        M0 = pt.M.copy()
        left = [(30 + 0.3 * y, y) for y in range(12, 37, 4)]
        right = [(110 - 0.3 * y, y) for y in range(12, 37, 4)]
        pt.updateTransformParams(left, right, "Default")
        assert not np.array_equal(pt.M, M0)
        want2 = warp_ref.warp_perspective(img, pt.M, (131, 37))
        assert not np.array_equal(want2, want)
        np.testing.assert_array_equal(pt.transformToBirdView(staged), want2)
        np.testing.assert_array_equal(pt.transformToFrontalView(staged), warp_ref.warp_perspective(img, pt.M_inv, (131, 37)))
        with pytest.raises(NotImplementedError, match="INTER_LINEAR"):
            pt.transformToBirdView(img, flags=0)         # cv2.INTER_NEAREST
        pt.close()                                       # releases the handle and the frame buffer; the next call creates them again
        assert pt._warp is None and pt._warp_src is None
        np.testing.assert_array_equal(pt.transformToBirdView(img), want2)
    finally:
        pt.close(); pt.close()                           # idempotent
        sbuf.free()


def test_error_paths_return_errors(G):
    L, PP, _ = G
    lib = L.lib()
    h = C.c_void_p()
    for bad in (L.WarpParams(0, 70, 37, 131), L.WarpParams(45, 70, 37, 0)):
        assert lib.adas_warp_create(C.byref(bad), 1, C.byref(h)) == -1            # ADAS_ERR_INVALID
    p = L.WarpParams(45, 70, 37, 131)
    assert lib.adas_warp_create(C.byref(p), 0, C.byref(h)) == -1
    w = PP.PerspectiveWarp((45, 70), (37, 131), 2)
    sbuf = L.DeviceBuffer(3 * 45 * 70 * 3)
    try:
        assert lib.adas_warp_run(w.h, sbuf.ptr, None, 3, None) == -1              # batch above max_batch: refused before any launch
        assert lib.adas_warp_run(w.h, sbuf.ptr, None, 0, None) == -1
        assert lib.adas_warp_run(w.h, None, None, 1, None) == -1
        # _lib.AdasError, a RuntimeError (the package may be loaded under two module names, so match the message, not the class)
        with pytest.raises(RuntimeError, match="libadas_hip error -1: adas_warp_fetch: no run has written"):
            w.fetch(0)                                                           # nothing has written the handle's buffer yet
        with pytest.raises(RuntimeError, match="libadas_hip error -1: adas_warp_set_matrix: the matrix is singular"):
            w.set_matrix(np.zeros((3, 3)))
        sbuf.upload(np.full((3, 45, 70, 3), 7, np.uint8))
        w.run(sbuf.ptr, 1)                                                       # identity matrices: frame 0 of the buffer is written
        assert w.fetch(0).shape == (37, 131, 3)
        with pytest.raises(RuntimeError, match="libadas_hip error -1: adas_warp_fetch: frame 1 .* never written"):
            w.fetch(1)                                                           # no run has reached frame 1: not uninitialised memory with ADAS_OK
        w.run(sbuf.ptr, 2)
        assert w.fetch(1).shape == (37, 131, 3)
    finally:
        w.close(); sbuf.free()
