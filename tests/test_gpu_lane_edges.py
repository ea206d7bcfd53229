"""GPU: the lane code that only hipcc compiles, on the inputs where it can go wrong without tests/test_gpu_post.py noticing: tied grid
maxima and tied existence logits, valid counts on the edge of every count rule, heads of 7 and 16 lanes, every local_width, block
loops of one to seven trips, UFLD v1 "no lane" ties, ego lanes of 0 .. 128 points fitted by a 64-lane team on frames of 256 .. 2397
rows, frames above 0 of a batch and handles used again with fewer points.  tests/hostemu compiles csrc/post_core.h and lane_core.h
with one thread: there ADAS_PAR_FOR is a plain loop, lane_team_sum the identity, lane_team_sync empty, bt_compact a `for`, and no
barrier matters, so the CPU suite reaches none of this.  The references are oracle/ufld_decode.py (process_output per frame,
process_output_v1) and test_hostemu_logic._geometry_reference under check_geometry, unchanged.  The exact head family (every softmax
tap 0 or 1/k) is compared bit for bit; the mixed family under the project's rule of +-1 px on at most 2 coordinates of a frame, the
count printed (measured on MI355X: 0 on each of the 113 mixed frames; the host emulation gives 0 too).  The cases come from tests/lane_cases.py; tests/test_lane_cases_cpu.py shows that each is sound and would tell a changed
tie rule apart.

device path -> cases
  ufld_decode_kernel, trips of the 640-thread loop    v2 (2,1,2,1): 8 .. 32 items, one partial trip;  (200,72,100,81) NL 4: 612, the last single
                                                      trip;  NL 7: 1071, two trips;  (200,128,100,128) NL 16: 4096, seven trips
  ufld1_decode_kernel, trips of the 256-thread loop   v1 (33,64): 256 items, the last single trip;  (17,65): 260, the first second trip;  (17,128): 512
  argmax scan: first maximum, unrolled body and tail  every exact v2 case: two or three maxima per column more than 2*lw cells apart, the first on cell 0, 1,
                                                      G-2, G-1, a group's last cell 8j, the next group's first cell 8j+1, the tail (G = 10, 12, 19, 26, 100,
                                                      200 have a tail, G = 9 and 17 none, G = 2 no body);  every mixed case (a tenth of the cells tie at 8)
  window clamped at m = 0 and m = G-1                 exact v2 cases with lw >= 1: first maxima on cells 0, 1, G-2, G-1 and flat columns (argmax 0)
  local_width 0, 2, 3 (v[8] holds up to 7 taps)       every v2 shape x num_lanes at lw = 0, 1, 2, 3;  G = 2 and G = 9 are narrower than the window of lw = 3
  existence ties mean "absent"                        every v2 case: the lanes below their count edge hold tied pairs, one more present anchor would pass
  cnt > R/2, cnt > C/4, n > 2 at their edges          every v2 case: counts floor(R/2) | +1 and floor(C/4) | +1;  R = 5, 7 odd, C = 9, 81, 1 not divisible by 4;
                                                      (10,7,9,4): counts 2 | 3 on the side lanes, `lane_cnt == 2, detected == False`
  num_lanes above 4 (stride num_lanes, lanes >= 4)    every v2 shape at NL = 7 and 16: lanes 4 .. NL-1 carry maxima and full existence
  ADAS_UFLD_MAXPTS points on a lane                   test_v2_batch (200,128,100,128): every anchor of frame 1 valid, 128 points on all four lanes;  v1 (17,128) "tie"
  v1: cell G equals the best real cell                every v1 case, role "tie" (and every second calm anchor of the other roles)
  v1: nz > 2 at 2 and 3                               every v1 case, roles "two" and "three";  (3,3) and (4,3): "half" leaves 2 non-zero anchors
  v1: "no lane" on the first K/2 anchors              every v1 case, role "half"
  v1: set_source_size after create                    every v1 case: (1280,720) at create, then (1640,590) and (333,777) on the live handle, and (333,777) at create
  v1: K up to 128, G from 3                           v1 (17,128);  (3,3)
  lane_polyfit2 as a 64-lane team: wave_allreduce_u64, the i > k row split
                                                      every geometry case with min(nL, nR) >= 3 (rows 0..2 in lanes 0..2);  direction cases;  geometry batch
  teams with idle lanes, full, wrapped                point counts 3, 10, 11, 12, 20, 63 (idle lanes);  64 (full);  65, 127, 128 (wrapped)
  two fits side by side in waves 0 and 1              (nL, nR) = (12,64) (63,64) (64,65) (65,20) (128,3) (11,128): the teams end at different times
  the second fit over Hb rows                         Hb = 720, 721, 1080, 2397 (the largest create accepts: 150 KB of LDS)
  refit gate nL > 10 && nR > 10                       (10,11) (11,10) (11,11) with adjust on;  every case with adjust off
  estimate gate Hb > 719                              frames (1279,719) (456,256) (455,257): no estimate;  (1280,720): estimate
  estimate gate nL >= 3 && nR >= 3                    (3,3) (128,3);  test_fewer_than_three_points: 0, 1, 2 points on either lane
  resample filters y >= min(lane ys), x >= 0          every refit case: the lanes start on different rows, the left lane leaves the image before the bottom row
  bt_compact, ballot form, over H samples             refit cases at H = 256, 257, 719, 720, 721, 1080, 2397
  direction: bend on both sides of +-0.00015, BL[0] <= BL[nL/2], BR[0] >= BR[nR/2] at equality
                                                      test_direction_case: eight cases, L, R, F by the threshold, F by the comparison
  frames above 0 of a batch, ufld_pack_kernel and lane_geometry_pack_kernel with frame > 0
                                                      test_v2_batch, test_v1_batch, test_geometry_batch (run and run_matrices, three homographies)
  a handle reused with fewer points than before       second launch of test_v2_batch and test_geometry_batch;  the geometry handles, shared by all cases of a frame
  create-time limits (lane_lds_bytes, 150 KB)         test_create_limits: 2398 rows -> ADAS_ERR_CAPACITY, 7 and 4321 -> ADAS_ERR_INVALID;  frame (4260,2397) runs"""
import numpy as np
import pytest

import lane_cases as LC
import test_hostemu_logic as TH
from oracle import ufld_decode
from test_lane_cases_cpu import _ids, check_decode, check_few, check_v1_roles

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_CAPACITY = -1, -5


@pytest.fixture(scope="module")
def G():
    import gpu_api
    assert gpu_api.L.lib().adas_device_count() > 0, "no HIP device"
    return gpu_api


# ------------------------------------------------------------------------------------------------ UFLD v2
@pytest.mark.parametrize("shape,nl,lw,family", LC.V2_CASES, ids=_ids)
def test_v2_case(G, shape, nl, lw, family):
    outs, cfg, (W, H), counts = LC.v2_case(shape, nl, lw, family)
    want = ufld_decode.process_output(outs, cfg, W, H, lw)
    check_decode(G.ufld(outs, cfg, W, H, lw), want, family, "gpu v2 %s" % _ids((shape, nl, lw)))


@pytest.mark.parametrize("shape,nl,lw", LC.V2_BATCHES, ids=_ids)
def test_v2_batch(G, shape, nl, lw):
    """Three different frames per launch on a handle of max_batch = 3, every frame fetched and compared with the oracle called per frame;
    the second launch on the same handle leaves fewer points in slot 1 than the first."""
    launches, cfg, (W, H) = LC.v2_batch(shape, nl, lw)
    ud = G.PP.UfldDecode(shape[0], shape[1], shape[2], shape[3], W, H, cfg.row_anchor, cfg.col_anchor, lw, max_batch=3, num_lanes=nl)
    try:
        for n, (outs, families) in enumerate(zip(launches, LC.V2_BATCH_FAMILIES)):
            got = ud.run_host(outs)
            assert len(got) == 3
            for b in range(3):
                want = ufld_decode.process_output(LC.frame_of(outs, b), cfg, W, H, lw)
                check_decode(got[b], want, families[b], "gpu v2 batch %s launch %d frame %d" % (_ids((shape, nl, lw)), n, b))
    finally:
        ud.close()


# ------------------------------------------------------------------------------------------------ UFLD v1
def _v1_handle(G, cfg, src, max_batch=1):
    return G.PP.Ufld1Decode(cfg.griding_num, cfg.cls_num_per_lane, cfg.img_w, cfg.img_h, LC.V1_INPUT[0], LC.V1_INPUT[1], src[0], src[1],
                            cfg.row_anchor, max_batch=max_batch)


@pytest.mark.parametrize("shape,family", LC.V1_CASES, ids=_ids)
def test_v1_case(G, shape, family):
    head, roles, cfg = LC.v1_case(shape, family)
    iw, ih = LC.V1_INPUT
    ud = _v1_handle(G, cfg, LC.V1_SOURCES[0])
    try:
        for n, src in enumerate(LC.V1_SOURCES):
            if n:
                ud.set_source_size(*src)                     # on the live handle
            want = ufld_decode.process_output_v1(head, cfg, iw, ih, src[0], src[1])
            check_v1_roles(want, roles, shape[1])
            check_decode(ud.run_host(head)[0], want, family, "gpu v1 %s %s" % (_ids(shape), _ids(src)))
    finally:
        ud.close()
    ud = _v1_handle(G, cfg, LC.V1_SOURCES[2])                # the same size through create
    try:
        check_decode(ud.run_host(head)[0], want, family, "gpu v1 %s %s at create" % (_ids(shape), _ids(LC.V1_SOURCES[2])))
    finally:
        ud.close()


def test_v1_batch(G):
    heads, roles, cfg = LC.v1_batch()
    ud = _v1_handle(G, cfg, (1280, 720), max_batch=3)
    try:
        got = ud.run_host(heads)
        assert len(got) == 3
        for b in range(3):
            want = ufld_decode.process_output_v1(heads[b], cfg, LC.V1_INPUT[0], LC.V1_INPUT[1], 1280, 720)
            check_decode(got[b], want, "mixed" if b == 1 else "exact", "gpu v1 batch frame %d" % b)
    finally:
        ud.close()


# ------------------------------------------------------------------------------------------------ lane geometry
@pytest.fixture(scope="module")
def slots(G):
    """A decode handle of three frame slots that only carries uploaded points."""
    cfg = ufld_decode.ModelConfig("culane")
    ud = G.PP.UfldDecode(200, 72, 100, 81, 1280, 720, cfg.row_anchor, cfg.col_anchor, 1, max_batch=3)
    yield ud
    ud.close()


@pytest.fixture(scope="module")
def geometry(G):
    """One LaneGeometry handle of three frames per frame size, shared by every case of that size."""
    made = {}

    def get(wh):
        if wh not in made:
            made[wh] = G.PP.LaneGeometry(wh[1], wh, np.eye(3), True, max_batch=3)
        return made[wh]
    yield get
    for lg in made.values():
        lg.close()


def _run_geometry(G, slots, lg, lanes, status, M, adjust):
    slots.upload(lanes, status, frame=0)
    lg.set_matrix(M)
    lg.run(slots, adjust)
    return G.lane_fetch(lg, 0)


@pytest.mark.parametrize("adjust", [True, False], ids=["adjust", "plain"])
@pytest.mark.parametrize("wh,counts", LC.GEO_CASES, ids=_ids)
def test_geometry_case(G, slots, geometry, wh, counts, adjust):
    W, H = wh
    lanes, status = LC.geo_lanes(wh, counts)
    M = LC.geo_matrix(wh, lanes)
    got = _run_geometry(G, slots, geometry(wh), lanes, status, M, adjust)
    TH.check_geometry(got, TH._geometry_reference(lanes, status, W, H, M, adjust))
    if got["direction"] is None:
        assert got["raw"] == (0.0, 0.0)


@pytest.mark.parametrize("name", sorted(LC.DIR_CASES))
def test_direction_case(G, slots, geometry, name):
    lanes, status = LC.dir_lanes(name)
    W, H = LC.DIR_WH
    want = TH._geometry_reference(lanes, status, W, H, np.eye(3), False)
    assert want[3] == LC.DIR_CASES[name][3]
    TH.check_geometry(_run_geometry(G, slots, geometry(LC.DIR_WH), lanes, status, np.eye(3), False), want)


@pytest.mark.parametrize("counts", LC.FEW_COUNTS, ids=_ids)
def test_fewer_than_three_points(G, slots, geometry, counts):
    """The project's rule, not the reference's (see test_lane_cases_cpu.check_few): fewer than three points on an ego lane give no
    estimate -- direction None, curvature and offset 0.0 -- and the bird-view points and the area polygon are still written.  The slot
    and the handle held a full estimate just before, so the zeros are this launch's."""
    wh = (1280, 720)
    full, full_status = LC.geo_lanes(wh, (64, 65))
    M = LC.geo_matrix(wh)
    before = _run_geometry(G, slots, geometry(wh), full, full_status, M, True)
    assert before["direction"] is not None and before["raw"][0] != 0.0 and before["raw"][1] != 0.0
    lanes, status, area = LC.few_lanes(counts)
    check_few(_run_geometry(G, slots, geometry(wh), lanes, status, M, True), lanes, status, area, M, wh)


def test_geometry_batch(G, slots, geometry):
    """Three frames in slots 0..2, one launch of run() with the handle's matrix and one of run_matrices() with three homographies in a
    device table, every frame fetched; then again with shorter lanes in slot 1."""
    launches, (W, H), Ms = LC.geo_batch()
    lg = geometry((W, H))
    table = G.L.DeviceBuffer.from_array(np.ascontiguousarray(np.stack([np.asarray(m, np.float64).reshape(9) for m in Ms])))
    try:
        for n, frames in enumerate(launches):
            for b, (lanes, status) in enumerate(frames):
                if n == 0 or b == 1:
                    slots.upload(lanes, status, frame=b)
            lg.set_matrix(Ms[0])
            lg.run(slots, True, batch=3)
            for b, (lanes, status) in enumerate(frames):
                TH.check_geometry(G.lane_fetch(lg, b), TH._geometry_reference(lanes, status, W, H, Ms[0], True))
            lg.run_matrices(slots, table.ptr, True, batch=3)
            for b, (lanes, status) in enumerate(frames):
                TH.check_geometry(G.lane_fetch(lg, b), TH._geometry_reference(lanes, status, W, H, Ms[b], True))
    finally:
        table.free()


@pytest.mark.parametrize("img_h,bird_h,code", [(2398, 720, ERR_CAPACITY), (720, 2398, ERR_CAPACITY), (2398, 2398, ERR_CAPACITY),
                                               (7, 720, ERR_INVALID), (720, 7, ERR_INVALID), (4321, 720, ERR_INVALID), (720, 4321, ERR_INVALID)])
def test_create_limits(G, img_h, bird_h, code):
    """Return codes of adas_lane_geometry_create, checked before any launch: max(img_h, bird_h) = 2397 is the largest the 150 KB of LDS
    hold (the (4260, 2397) cases run there), 2398 is a capacity error, heights outside [8, 4320] are invalid."""
    with pytest.raises(G.PP.L.AdasError) as e:          # (the package's own error class, whichever name it was imported under)
        G.PP.LaneGeometry(img_h, (1280, bird_h), np.eye(3))
    assert e.value.code == code
