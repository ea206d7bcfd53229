"""What the GPU tests of the overlay share (test_gpu_overlay.py, _objects.py, _tracks.py): the arrays of a batch as run_arrays takes them,
an overlay handle with its class colours, and one run_arrays launch into a guarded destination.  The expected images stay with each file."""
import collections
import importlib

import numpy as np
from conftest import load_pkg
import overlay_ref as ref

load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")

GUARD = 64          # bytes of 0xA5 on either side of a caller's destination: nothing may be written outside the frames
MAXP = L.UFLD_MAX_POINTS
FRAME_STAGES = 7 | 16 | 32 | 128   # every stage but the bird view's writes the frame and its flags

Result = collections.namedtuple("Result", "frames flags marks bird")


def noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _table(rows, cap, width, dtype, fill=0):
    """Per frame a list of `width`-tuples -> ([n][cap][width] filled with `fill` past each frame's rows, counts [n])."""
    tab, cnt = np.full((len(rows), cap, width), fill, dtype), np.zeros(len(rows), np.int32)
    for f, r in enumerate(rows):
        a = np.asarray(r, np.float64 if np.dtype(dtype).kind == "f" else np.int64).reshape(-1, width)
        tab[f, :len(a)], cnt[f] = a, len(a)
    return tab, cnt


class Scene:
    """Per-frame geometry of a batch.  Lanes, polygon and distance points are always there; `parts` names what else the scene holds and
    uploads: "style" (area on / off, offset type and area colour per frame; without it every area is on and the two pointers are null),
    "bird" (the bird view's lanes), "boxes" (detections and tracks), "trajectories" (per track its boxes, oldest first)."""

    def __init__(self, n, parts=(), det_cap=12, trk_cap=8, dist_cap=8, poly_cap=48):
        self.n, self.parts, self.det_cap, self.trk_cap, self.dist_cap, self.poly_cap = n, tuple(parts), det_cap, trk_cap, dist_cap, poly_cap
        self.lanes = [[[] for _ in range(4)] for _ in range(n)]
        self.poly = [[] for _ in range(n)]
        self.dist = [[] for _ in range(n)]
        self.area = [1] * n
        self.offset = [ref.OFFSET_UNKNOWN] * n
        self.colour = [ref.AREA_COLOR] * n
        self.bird = [[[] for _ in range(4)] for _ in range(n)]
        self.dets = [[] for _ in range(n)]          # (xmin, ymin, xmax, ymax, class)
        self.trks = [[] for _ in range(n)]          # (t, l, w, h, class)
        self.trajs = [[] for _ in range(n)]         # per track its boxes, oldest first

    @staticmethod
    def _lane_table(frames):
        pts, cnt = np.zeros((len(frames), 4, MAXP, 2), np.int32), np.zeros((len(frames), 4), np.int32)
        for f, lanes in enumerate(frames):
            for l in range(4):
                a = np.asarray(lanes[l], np.int64).reshape(-1, 2)
                pts[f, l, :len(a)], cnt[f, l] = a, len(a)
        return pts, cnt

    def upload(self):
        """The keyword arguments of LaneOverlay.run_arrays, device pointers into buffers the scene keeps until free()."""
        n, caps = self.n, dict(poly_cap=self.poly_cap, dist_cap=self.dist_cap)
        a = dict(area_status=np.array(self.area, np.int32))
        a["lane_points"], a["lane_counts"] = self._lane_table(self.lanes)
        a["poly"], a["poly_counts"] = _table(self.poly, self.poly_cap, 2, np.int32)
        a["dist_points"], a["dist_counts"] = _table(self.dist, self.dist_cap, 2, np.int32)
        if "style" in self.parts:
            a.update(offset_type=np.array(self.offset, np.int32), area_bgr=np.array(self.colour, np.uint8))
        if "bird" in self.parts:
            a["bird_points"], a["bird_counts"] = self._lane_table(self.bird)
        if "boxes" in self.parts:      # rows past a frame's count hold boxes (and full rings) that would show if they were drawn
            caps.update(det_cap=self.det_cap, trk_cap=self.trk_cap)
            det, a["det_counts"] = _table(self.dets, self.det_cap, 5, np.int32, 7)
            trk, a["trk_counts"] = _table(self.trks, self.trk_cap, 5, np.float64, 9.0)
            a["det_xyxy"], a["det_cls"] = np.ascontiguousarray(det[:, :, :4]), np.ascontiguousarray(det[:, :, 4])
            a["trk_tlwh"], a["trk_cls"] = np.ascontiguousarray(trk[:, :, :4]), np.ascontiguousarray(trk[:, :, 4].astype(np.int32))
            for f in range(n):
                a["det_cls"][f, a["det_counts"][f]:] = 0
                a["trk_cls"][f, a["trk_counts"][f]:] = 0
        if "trajectories" in self.parts:
            tr, tl = np.full((n, self.trk_cap, 30, 4), 20.0, np.float64), np.full((n, self.trk_cap), 30, np.int32)
            for f in range(n):
                assert len(self.trajs[f]) == len(self.trks[f])
                for k, t in enumerate(self.trajs[f]):
                    t = np.asarray(t, np.float64).reshape(-1, 4)
                    assert len(t) <= 30
                    tr[f, k, :len(t)], tl[f, k] = t, len(t)
            a["traj"], a["traj_len"] = tr, tl
        self.bufs = {k: L.DeviceBuffer.from_array(v) for k, v in a.items()}
        kw = {k: b.ptr for k, b in self.bufs.items() if k not in ("traj", "traj_len")}
        if "trajectories" in self.parts:
            kw["trajectories"] = (self.bufs["traj"].ptr, self.bufs["traj_len"].ptr)
        return dict(kw, **caps)

    def free(self):
        for b in self.bufs.values():
            b.free()


def make_overlay(n, h, w, bird_hw=None, det_table=None, trk_table=None, **style):
    ov = PP.LaneOverlay((h, w), bird_hw, n, **style)
    if det_table is not None:
        ov.set_class_colors("detections", det_table)
    if trk_table is not None:
        ov.set_class_colors("tracks", trk_table)
    return ov


def run(scene, src, stages=7, offset=16, in_place=False, own=False, bird=None, ov=None, **okw):
    """One run_arrays launch over the batch -> Result(frames, flags, marks, bird image).  A caller's destination sits at `offset` inside a
    canvas of 0xA5; own=True draws into the handle's buffer.  ov: the handle to use (else one made from okw and closed again)."""
    n, h, w = src.shape[:3]
    mine = ov is None
    if mine:
        ov = make_overlay(n, h, w, bird.shape[1:3] if bird is not None else None, **okw)
    kw = scene.upload()
    nbytes = src.nbytes
    canvas = np.full(nbytes + 2 * GUARD, 0xA5, np.uint8)
    if in_place:
        canvas[offset:offset + nbytes] = src.reshape(-1)
    dbuf = L.DeviceBuffer.from_array(canvas)
    sbuf = L.DeviceBuffer.from_array(src)
    bbuf = L.DeviceBuffer.from_array(bird) if bird is not None else None
    try:
        dst = None if own else dbuf.ptr + offset
        ov.run_arrays(dst if in_place else sbuf.ptr, n, stages=stages, dst_ptr=dst, bird_ptr=bbuf.ptr if bbuf else None, **kw)
        L.check(L.lib().adas_synchronize())
        if own:
            got = np.stack([ov.fetch(f) for f in range(n)])
            raw = np.empty_like(got)
            L.check(L.lib().adas_memcpy_d2h(L.ptr(raw), ov.device_view(), raw.nbytes))
            assert np.array_equal(raw, got)
        else:
            back = dbuf.download(canvas.shape, np.uint8)
            assert (back[:offset] == 0xA5).all() and (back[offset + nbytes:] == 0xA5).all(), "write outside the destination"
            got = back[offset:offset + nbytes].reshape(src.shape)
        assert np.array_equal(sbuf.download(src.shape, np.uint8), src), "the caller's frames were written"
        flags = [ov.flags(f) for f in range(n)] if stages & FRAME_STAGES else [0] * n
        marks = [ov.track_marks(f) for f in range(n)] if stages & 128 else [[] for _ in range(n)]
        return Result(got, flags, marks, bbuf.download(bird.shape, np.uint8) if bbuf else None)
    finally:
        if mine:
            ov.close()
        scene.free(); dbuf.free(); sbuf.free()
        if bbuf:
            bbuf.free()
