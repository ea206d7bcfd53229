"""GPU: the per-stream adaptive bird view (csrc/birdview_kernels.hip, adas_birdview_*), its two consumers
(adas_lane_geometry_run_matrices, adas_warp_run_device_matrices) and the three as optional stages of the fused step.
The kernel must equal the host build of the same text (tests/emu_birdview_api.py) bit for bit; the two consumers must equal the
existing single-matrix / host-matrix entry points bit for bit; the fused step must equal the components, captured or not."""
import gzip, importlib, json, os

import numpy as np
import pytest

from conftest import load_pkg, GOLDEN
import emu_birdview_api as E
import emu_warp_api
import warp_ref

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")

G = json.load(gzip.open(os.path.join(GOLDEN, "analysis.json.gz"), "rt"))["perspective"]
LEFT, RIGHT = [tuple(p) for p in G["left"]], [tuple(p) for p in G["right"]]
IMG = (1280, 720)
LANE_KW = dict(in_h=160, in_w=800, num_grid_row=100, num_cls_row=36, num_grid_col=50, num_cls_col=41)      # the reduced lane net of
LANE_CFG = dict(grid_row=100, cls_row=36, grid_col=50, cls_col=41, row_anchor=np.linspace(0.42, 1, 36),     # test_gpu_pipeline.py
                col_anchor=np.linspace(0, 1, 41))


def decoder(max_batch):
    return PP.UfldDecode(100, 36, 50, 41, 1280, 720, LANE_CFG["row_anchor"], LANE_CFG["col_anchor"], 1, max_batch)


def assert_state(got, emu, ctx=""):
    """A fetched stream state against the emulation's, every bit."""
    for f in ("src", "M", "M_inv", "M_warp"):
        assert np.asarray(got[f]).tobytes() == emu.state[f][0].tobytes(), (ctx, f, got[f], emu.state[f][0])
    assert (got["n_updates"], got["n_rejected"]) == (emu.n_updates, emu.n_rejected), ctx


def same_geometry(a, b, ctx=""):
    assert a["area_status"] == b["area_status"] and a["direction"] == b["direction"], ctx
    np.testing.assert_array_equal(a["area_points"], b["area_points"], err_msg=str(ctx))
    for li in range(4):
        np.testing.assert_array_equal(a["bird_points"][li], b["bird_points"][li], err_msg=str(ctx))
    assert a["curvature"] == b["curvature"] and a["offset"] == b["offset"], ctx


# ------------------------------------------------------------------------------------------------ the handle alone
def test_handle_three_streams_equals_the_emulation_bit_for_bit():
    """Stream 0 runs the reference's Default -> Top -> Bottom -> "Nonsense" trace, stream 1 never gets a request, stream 2 gets one on
    every run but its right ego lane is not detected."""
    dec = decoder(3)
    bv = PP.BirdView(IMG, 3, 3)
    emu = [E.BirdViewEmu(IMG) for _ in range(3)]
    lanes = [[], LEFT, RIGHT, []]
    dets = [[False, True, True, False], [False, True, True, False], [True, True, False, True]]
    for s in range(3):
        dec.upload(lanes, dets[s], s)
        assert_state(bv.fetch_stream(s), emu[s], ("initial", s))
    init = emu[1].state.copy()
    for k, step in enumerate(G["steps"]):
        bv.request(0, step["mode"])
        bv.request(2, "Default")
        assert bv.pending(2) == 1 and bv.pending(1) == 0
        bv.run(dec, 3, 1)
        want = [emu[0].frame(step["mode"], lanes, dets[0]), 0, emu[2].frame("Default", lanes, dets[2])]
        assert want == [0 if step["mode"] == "Nonsense" else 1, 0, 0]
        for s in range(3):
            assert_state(bv.fetch_stream(s), emu[s], (k, s))
            row = bv.fetch_frame(s)
            assert row["applied"] == want[s], (k, s)
            assert row["M"].tobytes() == emu[s].M.tobytes() and row["M_warp"].tobytes() == emu[s].M_warp.tobytes(), (k, s)
            assert bv.pending(s) == 0, (k, s)                       # consumed whether or not it was applied
        np.testing.assert_array_equal(bv.fetch_stream(0)["src"], np.float32(step["src"]))
    for s in (1, 2):                                                # never touched
        assert emu[s].state.tobytes() == init.tobytes()
    assert bv.fetch_stream(0)["n_updates"] == 3
    # a collapsed top edge is rejected on the device as in the emulation; reset brings a stream back
    bad = [[], [(560, 300), (500, 500), (430, 700)], [(520, 300), (700, 500), (860, 700)], []]
    dec.upload(bad, dets[0], 0)
    bv.request(0, "Default")
    bv.run(dec, 3, 1)
    assert emu[0].frame("Default", bad, dets[0]) == -1
    assert bv.fetch_frame(0)["applied"] == -1
    assert_state(bv.fetch_stream(0), emu[0], "rejected")
    assert bv.fetch_stream(0)["n_rejected"] == 1
    bv.request(1, "Top")
    bv.reset(-1)
    for s in range(3):
        assert bv.fetch_stream(s)["M"].tobytes() == init["M"][0].tobytes() and bv.pending(s) == 0
        assert bv.fetch_stream(s)["n_updates"] == 0 and bv.fetch_stream(s)["n_rejected"] == 0
    bv.close(); dec.close()


def test_frames_of_a_stream_are_walked_in_temporal_order():
    """n_streams = 2, n_frames = 3, a request on stream 1 only: it lands on that stream's first frame (index 0 * 2 + 1) and the
    stream's later frames (3, 5) carry the new matrix; stream 0's frames (0, 2, 4) keep the old one."""
    dec = decoder(6)
    bv = PP.BirdView(IMG, 2, 6)
    old, new = E.BirdViewEmu(IMG), E.BirdViewEmu(IMG)
    lanes, det = [[], LEFT, RIGHT, []], [False, True, True, False]
    for f in range(6):
        dec.upload(lanes, det, f)
    bv.request(1, "Default")
    bv.run(dec, 2, 3)
    assert new.frame("Default", lanes, det) == 1 and new.M.tobytes() != old.M.tobytes()
    rows = [bv.fetch_frame(f) for f in range(6)]
    assert [r["applied"] for r in rows] == [0, 1, 0, 0, 0, 0]
    for f in (1, 3, 5):
        assert rows[f]["M"].tobytes() == new.M.tobytes() and rows[f]["M_warp"].tobytes() == new.M_warp.tobytes(), f
    for f in (0, 2, 4):
        assert rows[f]["M"].tobytes() == old.M.tobytes() and rows[f]["M_warp"].tobytes() == old.M_warp.tobytes(), f
    assert_state(bv.fetch_stream(0), old, "stream 0")
    assert_state(bv.fetch_stream(1), new, "stream 1")
    # _lib.AdasError, a RuntimeError (the package may be loaded under two module names, so match the message, not the class)
    with pytest.raises(RuntimeError, match="adas_birdview_run: bad argument"):
        bv.run(dec, 2, 4)                                           # 8 frames: more than the tables hold
    bv.close(); dec.close()


# ------------------------------------------------------------------------------------------------ the two consumers
def test_run_matrices_equals_run_after_set_matrix_per_frame():
    dec = decoder(3)
    mats = []
    e = E.BirdViewEmu(IMG)
    for mode in ("Default", "Top", "Bottom"):
        e.update(LEFT, RIGHT, mode)
        mats.append(e.M)
    assert len({m.tobytes() for m in mats}) == 3
    curvy = G["curvy"]
    frames = [[[], LEFT, RIGHT, []], [[], [tuple(p) for p in curvy["left"]], [tuple(p) for p in curvy["right"]], []],
              [[(100, 400), (90, 500), (80, 600)], LEFT[::2], RIGHT[::3], []]]
    for f, lanes in enumerate(frames):
        dec.upload(lanes, [len(l) > 2 for l in lanes], f)
    tab = L.DeviceBuffer.from_array(np.stack(mats).reshape(3, 9))
    many = PP.LaneGeometry(720, IMG, mats[0], True, 3)
    one = PP.LaneGeometry(720, IMG, mats[0], True, 3)
    for adjust in (True, False):
        many.run_matrices(dec, tab.ptr, adjust, 3)
        got = [many.fetch(f) for f in range(3)]
        for f in range(3):                                          # the existing path is the yardstick
            one.set_matrix(mats[f])
            one.run(dec, adjust, 3)
            same_geometry(got[f], one.fetch(f), (adjust, f))
        assert got[0]["direction"] is not None and got[0]["area_status"]
    one.set_matrix(mats[0])                                         # frame 1 really read ITS row: matrix 0 gives other points there
    one.run(dec, False, 3)
    assert not np.array_equal(one.fetch(1)["bird_points"][1], got[1]["bird_points"][1])
    many.close(); one.close(); tab.free(); dec.close()


def test_run_device_matrices_equals_run_and_the_restatement():
    """Source 37x53, destination 29x41 (width % 4 == 1: the row tail and the unaligned store path), batch 3; the third matrix sends part
    of the image outside the source."""
    sh, sw, dh, dw = 37, 53, 29, 41
    src = np.random.default_rng(5).integers(0, 256, (3, sh, sw, 3), dtype=np.uint8)
    pt = A.PerspectiveTransformation((dw, dh))
    mw = [emu_warp_api.invert3x3(pt.M), emu_warp_api.invert3x3(pt.M_inv), np.array([1.0, 0.08, -9.5, -0.05, 1.0, 6.25, 0.0, 0.0, 1.0])]
    sbuf = L.DeviceBuffer.from_array(src)
    tab = L.DeviceBuffer.from_array(np.stack(mw).reshape(3, 9))
    a = PP.PerspectiveWarp((sh, sw), (dh, dw), 3)
    b = PP.PerspectiveWarp((sh, sw), (dh, dw), 3)
    a.run_device_matrices(sbuf.ptr, tab.ptr, 3)
    for f in range(3):
        b.set_matrix(mw[f], f, inverse=True)
    b.run(sbuf.ptr, 3)
    outside = 0
    for f in range(3):
        got, want = a.fetch(f), b.fetch(f)
        ref = warp_ref.warp_perspective(src[f], mw[f], (dw, dh), inverse=True)
        np.testing.assert_array_equal(got, want, err_msg="frame %d vs adas_warp_run" % f)
        np.testing.assert_array_equal(got, ref, err_msg="frame %d vs warp_ref" % f)
        outside += int((ref.reshape(-1, 3).max(1) == 0).sum())
    assert outside > 20 and int((warp_ref.warp_perspective(src[2], mw[2], (dw, dh), inverse=True) > 0).sum()) > 1000
    # into a caller's buffer as well, and a batch the handle does not hold is refused
    out = L.DeviceBuffer(3 * dh * dw * 3)
    a.run_device_matrices(sbuf.ptr, tab.ptr, 3, dst_ptr=out.ptr)
    L.check(L.lib().adas_synchronize())
    np.testing.assert_array_equal(out.download((3, dh, dw, 3), np.uint8), np.stack([b.fetch(f) for f in range(3)]))
    with pytest.raises(RuntimeError, match="adas_warp_run_device_matrices: bad argument"):
        a.run_device_matrices(sbuf.ptr, tab.ptr, 4)
    a.close(); b.close(); sbuf.free(); tab.free(); out.free()


# ------------------------------------------------------------------------------------------------ the fused step
class PrescribedLanes:
    """A weight source for the lane net: every weight zero, and the last layer's bias chosen so that the decoder's arg-maxima fall where
    wanted -- both ego lanes exist on every row anchor, at grid cells that spread towards the bottom of the frame.  The network's
    output is then its bias whatever the input: area_status holds by construction."""

    def __init__(self):
        gr, r, gc, c = 100, 36, 50, 41
        loc_row = np.zeros((gr, r, 4), np.float32)
        exist_row = np.zeros((2, r, 4), np.float32)
        for k in range(r):
            loc_row[int(round(44 - 0.4 * k)), k, 1] = 10.0
            loc_row[int(round(55 + 0.45 * k)), k, 2] = 10.0
        exist_row[1, :, 1:3] = 5.0
        self.bias = np.concatenate([loc_row.reshape(-1), np.zeros(gc * c * 4, np.float32), exist_row.reshape(-1), np.zeros(2 * c * 4, np.float32)])

    def __call__(self, name, shape, kind, fill=None):
        if name == "cls.3.bias":
            assert tuple(shape) == self.bias.shape
            return self.bias
        return np.zeros(shape, np.float32)


@pytest.fixture(scope="module")
def lane_model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bv") / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=PrescribedLanes(), **LANE_KW).save(path)
    return path


@pytest.fixture(scope="module")
def det_model(tmp_path_factory):
    return M.build("yolov8n").save(str(tmp_path_factory.mktemp("bvd") / "d.hipm"))


@pytest.mark.parametrize("micro_batch", [1, 2])
def test_pipeline_graph_eager_and_components_agree(lane_model, det_model, micro_batch):
    import bench
    S, B = 2, micro_batch
    F = S * B
    cam = [bench.cam_frames(F, 300 + i) for i in range(2)]
    dev = [L.DeviceBuffer.from_array(c) for c in cam]
    Mh = A.PerspectiveTransformation(IMG).M
    kw = dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, micro_batch=B,
              geometry=dict(bird_wh=IMG, M=Mh), birdview=dict(image=True))
    pg = PL.AdasPipeline(det_model, lane_model, use_graph=True, **kw)      # lane branch forked onto its own stream inside the capture
    pe = PL.AdasPipeline(det_model, lane_model, use_graph=False, **kw)
    bv = PP.BirdView(IMG, S, F)
    geo = PP.LaneGeometry(720, IMG, Mh, True, F)
    warp = PP.PerspectiveWarp((720, 1280), (720, 1280), F)
    d_M, d_Mw = bv.device_views()
    init = E.BirdViewEmu(IMG)
    emu = E.BirdViewEmu(IMG)
    for k, mode in enumerate(("Default", "Top", "Bottom")):
        d = dev[k % 2]
        for p in (pg, pe):
            p.request_transform(0, mode)                                   # between steps; the captured step is replayed as it is
            p.step_frames(d.ptr, (720, 1280), 0.6)
            p.sync()
        lanes, det = pg.decode.fetch(0)
        assert det[1] and det[2] and len(lanes[1]) == 36 and len(lanes[2]) == 36          # prescribed, not luck
        assert emu.frame(mode, lanes, det) == 1
        bv.request(0, mode)
        bv.run(pg.decode, S, B)
        geo.run_matrices(pg.decode, d_M, True, F)
        warp.run_device_matrices(d.ptr, d_Mw, F)
        for s in range(S):
            sg, se, sc = pg.birdview.fetch_stream(s), pe.birdview.fetch_stream(s), bv.fetch_stream(s)
            assert_state(sg, emu if s == 0 else init, (k, s, "graph"))
            assert_state(se, emu if s == 0 else init, (k, s, "eager"))
            assert_state(sc, emu if s == 0 else init, (k, s, "components"))
        for f in range(F):
            rg, re_, rc = pg.birdview.fetch_frame(f), pe.birdview.fetch_frame(f), bv.fetch_frame(f)
            assert rg["applied"] == re_["applied"] == rc["applied"] == (1 if f == 0 else 0), (k, f)
            want = emu if f % S == 0 else init
            for r in (rg, re_, rc):
                assert r["M"].tobytes() == want.M.tobytes() and r["M_warp"].tobytes() == want.M_warp.tobytes(), (k, f)
            assert pg.decode.fetch(f) == pe.decode.fetch(f)
            gg, ge, gc = pg.geometry.fetch(f), pe.geometry.fetch(f), geo.fetch(f)
            same_geometry(gg, ge, (k, f, "graph vs eager"))
            same_geometry(gg, gc, (k, f, "graph vs components"))
            assert gg["area_status"] and gg["direction"] is not None
            ig, ie, ic = pg.birdview_image(f), pe.birdview_image(f), warp.fetch(f)
            assert np.array_equal(ig, ie) and np.array_equal(ig, ic), (k, f)
            assert ig.shape == (720, 1280, 3) and int(ig.max()) > 0
    assert pg.birdview.fetch_stream(0)["n_updates"] == 3 and pe.birdview.fetch_stream(0)["n_updates"] == 3     # every request was applied
    assert pg.birdview.fetch_stream(1)["M"].tobytes() == init.M.tobytes()                                       # no request: initial matrix
    assert not np.array_equal(pg.geometry.fetch(0)["bird_points"][1], pg.geometry.fetch(1)["bird_points"][1])   # same lanes, other matrix
    # the image follows the stream's own matrix: frame 0 against the restatement on a few rows' worth of pixels is the warp's own test;
    # here it must differ between the re-anchored stream and the untouched one only through the matrix
    with pytest.raises(RuntimeError, match="no frame to warp") as ei:       # seam tensors with a warp attached
        pg.step(dev[0].ptr, dev[0].ptr)
    assert ei.value.code == -1                                              # ADAS_ERR_INVALID
    for o in (pg, pe, bv, geo, warp):
        o.close()
    for d in dev:
        d.free()


def test_points_only_stage_and_a_pipeline_without_it(lane_model):
    """birdview=dict(image=False): matrices and geometry only, and the seam-tensor step stays legal.  A pipeline created without
    birdview= fetches what the stand-alone geometry gives with the handle's single matrix, as before."""
    import bench
    S = 2
    cam = L.DeviceBuffer.from_array(bench.cam_frames(S, 411))
    Mh = A.PerspectiveTransformation(IMG).M
    kw = dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, use_graph=True, geometry=dict(bird_wh=IMG, M=Mh))
    plain = PL.AdasPipeline(None, lane_model, **kw)
    pts = PL.AdasPipeline(None, lane_model, birdview=dict(image=False), **kw)
    assert plain.birdview is None and plain.warp is None and pts.warp is None
    with pytest.raises(ValueError):
        plain.request_transform(0, "Default")
    pts.request_transform(1, "Bottom")
    for p in (plain, pts):
        p.step_frames(cam.ptr, (720, 1280), 0.6)
        p.sync()
    geo = PP.LaneGeometry(720, IMG, Mh, True, S)
    geo.run(plain.decode, True, S)
    for s in range(S):
        same_geometry(plain.geometry.fetch(s), geo.fetch(s), s)
    emu = E.BirdViewEmu(IMG)
    lanes, det = pts.decode.fetch(1)
    assert emu.frame("Bottom", lanes, det) == 1
    assert_state(pts.birdview.fetch_stream(1), emu, "points only")
    assert pts.birdview.fetch_frame(1)["applied"] == 1 and pts.birdview.fetch_frame(0)["applied"] == 0
    geo.set_matrix(emu.M)
    geo.run(pts.decode, True, S)
    same_geometry(pts.geometry.fetch(1), geo.fetch(1), "re-anchored stream")
    x = L.DeviceBuffer(S * 3 * 160 * 800 * 4)
    L.check(L.lib().adas_memcpy_h2d(x.ptr, L.ptr(np.zeros(S * 3 * 160 * 800, np.float32)), x.nbytes))
    pts.step(None, x.ptr)                                                   # no warp attached: seam tensors are fine
    pts.sync()
    assert pts.birdview.fetch_frame(1)["applied"] == 0 and pts.birdview.fetch_stream(1)["n_updates"] == 1
    with pytest.raises(ValueError):
        pts.birdview_image(0)
    with pytest.raises(ValueError):
        PL.AdasPipeline(None, lane_model, n_streams=1, src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, birdview=dict(image=False))
    for o in (plain, pts, geo):
        o.close()
    cam.free(); x.free()
