"""GPU: the ByteTrack code that only hipcc compiles, on the inputs where it can go wrong without tests/test_gpu_post.py noticing:
assignment problems on both sides of every solver size class in which neighbouring tracks compete for detections, exact cost ties,
empty sides, and the capacity rules.  tests/hostemu compiles csrc/track_core.h with one thread: there bt_assign is always the serial
bt_lap, block_argmin_unused a loop, bt_compact a `for`, and no barrier matters, so the CPU suite reaches none of this.  Every frame is
compared with the oracle under parity_checks.check_track_frame and BtHeader.err is asserted.  The oracle solves with scipy for the
contested and degenerate cases (tests/test_track_cases_cpu.py proves them free of ties), with lap_ref("first") -- the device's tie
rule restated -- for the tie scenes, under track_cases.CapOracle's capacity rules throughout.  The cases come from tests/track_cases.py.

device path -> cases
  bt_lap_wave<1>  (D + 1 <= 64)               contested (70, 63);  every degenerate and capacity case;  second and third associations
  bt_lap_wave<2>  (65 .. 128)                 contested (64, 64)  (100, 127);  tie scenes of 100 columns, dupdet-lo-100 in the second association
  bt_lap_wave<4>  (129 .. 256)                contested (128, 128)  (100, 130)  (255, 255);  tie scenes of 130 columns
  bt_lap_wave<8>  (257 .. 512)                contested (200, 256)  (511, 511);  tie scenes of 300 columns
  block bt_lap + block_argmin_unused          contested (512, 512): three partial passes of 256 threads;  (300, 513): T < D;  (600, 700);
                                              tie scenes of 600 columns
  first minimum: one 64-column group          every tie scene: columns (3, 9) and the neighbour pairs
  first minimum: higher column, lower lane    tie scenes: (40, 70) of 100;  (40, 128) of 130;  (40, 138) and (100, 290) of 300
  first minimum: one thread, two passes       tie scenes of 600: (10, 266);  two waves of one pass: (40, 138);  two passes: (300, 580)
  equal slack keeps the earlier path          duptrk-*: two identical tracks, one detection
  cost matrix in LDS                          (70, 63) (64, 64) on both capacities;  (100, 127) (128, 128) (100, 130) on (256, 256)
  cost matrix in HBM (BtStream.cost)          (255, 255) on both capacities;  everything above 7652 products on (1024, 1024)
  LDS carve of capacity (1024, 1024)          every contested case and tie scene (98.5 KB fixed + the cost matrix)
  bt_compact, ballot form                     every case: score bands of up to 875 rows (four trips of 256), pool, leftovers, new tracks,
                                              list algebra;  empty inputs in the degenerate cases
  T = 0 / D = 0 / both / no low band / unconfirmed alone / scores on the threshold
                                              degenerate cases, by name
  BT_ERR_TRACK_OVERFLOW                       track-overflow (8 slots, 12 candidates);  contested (255, 255) on (256, 256) from f1 on
  BT_ERR_DET_OVERFLOW                         det-overflow through update_device (count 12, max_dets 8);  update_host refuses
  BT_ERR_HIST_OVERFLOW                        hist-overflow (a ninth class)
  err sticky / cleared by reset / per stream  track-overflow, det-overflow;  the neighbour stream of every capacity case
  adas_bytetrack_update_device                test_update_device_entry: det_stride 300, count_stride 3, count_index 1, 2 of 3 streams
  adas_bytetrack_update_device_frames         test_update_device_frames: 3 frames x 2 streams, fetch_frame of every frame, reset between launches
  adas_bytetrack_fetch_trajectories           last frame of every contested case
  two handles of different capacity           test_two_capacities_live"""
import pytest

import lap_ref, parity_checks as pc, track_cases as TC
from oracle import bytetrack

pytestmark = pytest.mark.gpu
CASES_A = [(T, D, cap) for T, D in TC.CONTESTED for cap in TC.caps_of(T, D)]


@pytest.fixture(scope="module")
def G():
    import gpu_api
    assert gpu_api.L.lib().adas_device_count() > 0, "no HIP device"
    return gpu_api


@pytest.fixture(scope="module")
def trackers(G):
    """One two-stream tracker per capacity, reset before each use."""
    made = {}

    def get(cap):
        if cap not in made:
            made[cap] = G.PP.DeviceTracker(2, max_tracks=cap[0], max_dets=cap[1])
        made[cap].reset(-1)
        return made[cap]
    yield get
    for t in made.values():
        t.close()


def _run_host(G, trk, s, steps, want, ctx):
    """The steps through update_host on stream s, every frame against want[f] = (snapshot, err)."""
    f = 0
    for st in steps:
        if isinstance(st, str):
            trk.reset(s)
            continue
        trk.update_host(s, st["boxes"], st["scores"], st["ids"])
        got, err = G.track_fetch(trk, s)
        pc.check_track_frame(got, want[f][0], ctx=(ctx, f))
        assert err == want[f][1], (ctx, f, err, want[f][1])
        f += 1
    assert f == len(want)


def _untouched(G, trk, s):
    got, err = G.track_fetch(trk, s)
    assert got == dict(frame_id=0, count=0, tracked=[], lost=[]) and err == 0


# ------------------------------------------------------------------------------------------------ a. contested size-class scenes
@pytest.mark.parametrize("T,D,cap", CASES_A, ids=lambda v: str(v).replace(" ", ""))
def test_contested(G, trackers, T, D, cap):
    steps = TC.contested_case(T, D, cap)["steps"]
    want, ora = TC.expected(steps, cap)
    trk = trackers(cap)
    _run_host(G, trk, 1, steps, want, (T, D, cap))
    _untouched(G, trk, 0)
    got_tr, want_tr = trk.fetch_trajectories(1), TC.oracle_trajectories(ora)
    assert len(got_tr) == len(want_tr)
    for k, (g, w) in enumerate(zip(got_tr, want_tr)):
        assert g.tolist() == w.tolist(), (T, D, cap, k)


# ------------------------------------------------------------------------------------------------ b. tie scenes
@pytest.mark.parametrize("name", sorted(TC.tie_cases()))
def test_tie_scene(G, trackers, name, monkeypatch):
    steps, _ = TC.tie_cases()[name]
    monkeypatch.setattr(bytetrack, "lapjv_extended", lap_ref.first)
    want, _ = TC.expected(steps, TC.BIG)
    trk = trackers(TC.BIG)
    _run_host(G, trk, 0, steps, want, name)
    _untouched(G, trk, 1)


# ------------------------------------------------------------------------------------------------ c. degenerate shapes
@pytest.mark.parametrize("name", sorted(TC.degenerate_cases()))
def test_degenerate(G, trackers, name):
    steps = TC.degenerate_cases()[name]
    want, _ = TC.expected(steps, TC.DEFAULT)
    trk = trackers(TC.DEFAULT)
    _run_host(G, trk, 1, steps, want, name)
    _untouched(G, trk, 0)


# ------------------------------------------------------------------------------------------------ d. capacity
@pytest.mark.parametrize("name", sorted(TC.capacity_cases()))
def test_capacity(G, trackers, name):
    cap, steps, errs, entry = TC.capacity_cases()[name]
    want, _ = TC.expected(steps, cap)
    assert [e for _, e in want] == errs
    trk = trackers(cap)
    other = TC.degenerate_cases()["no-low-band"][0]                # the neighbour stream: a legal frame before and after
    want_other = TC.expected([other], cap)[0][0][0]
    trk.update_host(1, other["boxes"], other["scores"], other["ids"])
    if entry == "host":
        _run_host(G, trk, 0, steps, want, name)
    else:
        for f, st in enumerate(steps):
            n = len(st["scores"])
            if n > cap[1]:
                with pytest.raises(G.PP.L.AdasError) as e:          # (the package's own error class, whichever name it was imported under)
                    trk.update_host(0, st["boxes"], st["scores"], st["ids"])
                assert e.value.code == G.ERR_CAPACITY and "max_dets" in str(e.value)
                assert G.track_fetch(trk, 0)[0]["frame_id"] == f     # refused: no frame was consumed
            views, bufs = G.upload_det_slabs([st], det_stride=16, count_stride=3, count_index=1)
            trk.update_device(views, det_stride=16, n_streams=1, count_stride=3, count_index=1)
            got, err = G.track_fetch(trk, 0)
            for b in bufs:
                b.free()
            pc.check_track_frame(got, want[f][0], ctx=(name, f))
            assert err == want[f][1], (name, f, err)
    got, err = G.track_fetch(trk, 1)
    pc.check_track_frame(got, want_other, ctx=(name, "neighbour"))
    assert err == 0


def test_two_capacities_live(G, trackers):
    """A tracker keeps working after a smaller one was created beside it (both launch one kernel with their own LDS size)."""
    big = trackers(TC.BIG)
    small = G.PP.DeviceTracker(1, max_tracks=8, max_dets=8)
    steps = TC.contested_case(70, 63, TC.BIG)["steps"][:2]
    _run_host(G, big, 0, steps, TC.expected(steps, TC.BIG)[0], "big beside small")
    fr = TC.capacity_cases()["hist-overflow"][1][0]
    _run_host(G, small, 0, [fr], TC.expected([fr], (8, 8))[0], "small beside big")
    small.close()


# ------------------------------------------------------------------------------------------------ entry points
def test_update_device_entry(G):
    """adas_bytetrack_update_device from device arrays whose strides are not the counts: det_stride 300 over frames of up to 78 rows,
    the count in word 1 of 3, and 2 of the handle's 3 streams per launch; the third keeps its frame_id and lists."""
    a = TC.contested_case(70, 63, TC.DEFAULT)["steps"]
    b = TC.degenerate_cases()["no-dets"]
    c = TC.degenerate_cases()["no-low-band"][0]
    wa, wb = TC.expected(a, TC.DEFAULT)[0], TC.expected(b, TC.DEFAULT)[0]
    wc = TC.expected([c], TC.DEFAULT)[0][0][0]
    trk = G.PP.DeviceTracker(3)
    trk.update_host(2, c["boxes"], c["scores"], c["ids"])
    for f in range(4):
        views, bufs = G.upload_det_slabs([a[f], b[f]], det_stride=300, count_stride=3, count_index=1)
        trk.update_device(views, det_stride=300, n_streams=2, count_stride=3, count_index=1)
        for s, w in ((0, wa), (1, wb)):
            got, err = G.track_fetch(trk, s)
            pc.check_track_frame(got, w[f][0], ctx=("update_device", s, f))
            assert err == w[f][1] == 0
        for buf in bufs:
            buf.free()
        got, err = G.track_fetch(trk, 2)
        pc.check_track_frame(got, wc, ctx=("untouched stream", f))
        assert err == 0
    trk.close()


def test_update_device_frames(G, monkeypatch):
    """adas_bytetrack_update_device_frames: three frames of two streams per launch, stream 0 with the 130-column frame mid-batch, stream 1
    a tie scene; fetch_frame(s, f) is the oracle's message of that frame, fetch(s) the last; between two launches stream 1 is reset."""
    monkeypatch.setattr(bytetrack, "lapjv_extended", lap_ref.first)       # (f0..f3 of the contested scene are free of ties: scipy's answer)
    f0, f1, f2, f3 = TC.contested_case(100, 130, TC.DEFAULT)["steps"]
    tie = TC.tie_cases()["dupdet-100"][0]
    s0 = [f0, f1, f2, f3, f1, f2]
    s1 = tie + ["reset"] + tie
    w0, w1 = TC.expected(s0, TC.DEFAULT)[0], TC.expected(s1, TC.DEFAULT)[0]
    assert len(f1["scores"]) == 162 and sum(s > 0.5 for s in f1["scores"]) == 130
    trk = G.PP.DeviceTracker(2)
    for launch in range(2):
        if launch:
            trk.reset(1)
        slabs = []
        for f in range(3):
            slabs += [s0[3 * launch + f], tie[f]]                          # slab f * n_streams + s
        views, bufs = G.upload_det_slabs(slabs, det_stride=200, count_stride=3, count_index=1)
        trk.update_device_frames(views, det_stride=200, n_frames=3, n_streams=2, count_stride=3, count_index=1)
        for s, w in ((0, w0), (1, w1)):
            for f in range(3):
                got, err = G.track_fetch(trk, s, frame=f)
                pc.check_track_frame(got, w[3 * launch + f][0], ctx=("frames", launch, s, f))
                assert err == w[3 * launch + f][1] == 0
            got, err = G.track_fetch(trk, s)
            pc.check_track_frame(got, w[3 * launch + 2][0], ctx=("frames", launch, s, "live"))
            assert err == 0
            hdr, tracked, lost = trk.fetch_frame(s, 2)                     # the package wrapper reads the same message
            pc.check_track_frame(G.track_snapshot(hdr, tracked, lost), w[3 * launch + 2][0], ctx=("fetch_frame", launch, s))
        for b in bufs:
            b.free()
    trk.close()
