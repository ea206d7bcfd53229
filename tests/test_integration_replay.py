"""INTEGRATION.md section A, executed: the REFERENCE's unmodified YoloDetector / UltrafastLaneDetectorV2 on a swapped `coreEngine`.

CPU test, in two recorded halves that meet here.  The engine the reference's classes talk to replays what this repo's HipEngine exposed
and returned on an MI355X for one 1280x720 frame (tests/golden/dropin_replay.npz, recorded by tests/golden/record_dropin_replay.py).
What the reference's own classes made of that replay -- the calls they issued, `object_info`, `lane_info` -- is stored beside it
(tests/golden/dropin_replay_ref.json, written by `python tests/integration_replay.py tests/golden/dropin_replay.npz
tests/golden/dropin_replay_ref.json` where the reference tree exists; tests/integration_replay.py holds the replay engine and the
environment shims).  The reference's results must equal the device results recorded with them (ObjectDetector/core.py:73-91,
ObjectDetector/yoloDetector.py:74-80,159-168, ufldDetector/ultrafastLaneDetectorV2.py:82-95,183-194), and this repo's oracle
post-processing, run on the replayed tensors, must give the reference's results too.
"""
import json
import os

import numpy as np
import pytest

from conftest import ROOT

FIXTURE = os.environ.get("ADAS_REPLAY_FIXTURE") or os.path.join(ROOT, "tests", "golden", "dropin_replay.npz")
REF_RESULTS = os.path.join(ROOT, "tests", "golden", "dropin_replay_ref.json")


@pytest.fixture(scope="module")
def replayed():
    return json.load(open(REF_RESULTS)), dict(np.load(FIXTURE, allow_pickle=False))


def test_reference_classes_read_the_hip_engine_surface(replayed):
    got, fx = replayed
    # both suffix branches of the reference's dispatch (yoloDetector.py:74-77, ultrafastLaneDetectorV2.py:82-85) landed on the swapped engine,
    # and the tensors their own pre-processing built are bit for bit the ones the device pre-processing fed HipEngine
    assert [c["kind"] for c in got["calls"]] == ["det", "lane"]
    assert all(c["input_is_the_device_tensor"] for c in got["calls"]), got["calls"]
    assert got["det"]["engine_class"] == "ReplayEngine" and got["det"]["input_types"] == str(fx["det_engine_dtype"]) == "float32"
    assert got["det"]["input_shapes"] == [int(v) for v in fx["det_input_shape"]] == [1, 3, 640, 640]       # set_input_details, core.py:73-82
    assert got["det"]["output_names"] == [str(n) for n in fx["det_output_names"]]
    assert got["lane"]["input_shape"] == [int(v) for v in fx["lane_input_shape"]] == [1, 3, 320, 1600]
    assert got["lane"]["output_names"] == [str(n) for n in fx["lane_output_names"]] and len(got["lane"]["output_names"]) == 4   # :93-94
    assert str(fx["det_framework_type"]) == "hip" and "HIPExecutionProvider" in str(np.atleast_1d(fx["det_providers"])[0])


def test_reference_yolo_detector_on_replayed_engine_equals_device_results(replayed):
    """object_info of the reference's YoloDetector (its own letterbox, decode loop, inverse letterbox, fast_soft_nms, RectInfo) on the
    head HipEngine returned == the device path's object_info for the same frame: every field, exactly."""
    got, fx = replayed
    d = got["det"]
    assert d["all_rectinfo"] and len(d["xywh"]) == len(fx["det_xywh"]) >= 3
    np.testing.assert_array_equal(np.asarray(d["xywh"], np.float64).reshape(-1, 4), fx["det_xywh"])
    np.testing.assert_array_equal(np.asarray(d["conf"], np.float64), fx["det_conf"])
    assert d["label"] == [str(s) for s in fx["det_label"]]
    np.testing.assert_array_equal(np.asarray(d["xyxy_int"], np.int64).reshape(-1, 4), fx["det_xyxy_int"])      # RectInfo.tolist, core.py:18-23


def test_reference_lane_detector_on_replayed_engine_equals_device_results(replayed):
    """lane_info of the reference's UltrafastLaneDetectorV2 on HipEngine's four outputs == the device path's: same lanes found, same
    number of points per lane, coordinates within 1 px (the 3-tap softmax: NumPy's exp there, expf on the device), same ego-lane
    area decision and polygon (within 2 px: it is a least-squares refit of those points)."""
    got, fx = replayed
    l = got["lane"]
    assert l["status"] == [bool(s) for s in fx["lane_status"]] and sum(l["status"]) >= 1
    for i in range(4):
        want = fx["lane_points%d" % i].reshape(-1, 2)
        have = np.asarray(l["points"][i], np.int64).reshape(-1, 2)
        assert have.shape == want.shape, (i, have.shape, want.shape)
        assert np.abs(have - want).max(initial=0) <= 1, (i, np.abs(have - want).max())
    assert l["area_status"] == bool(fx["lane_area_status"])
    a, b = np.asarray(l["area_points"], np.int64).reshape(-1, 2), fx["lane_area_points"].reshape(-1, 2)
    assert a.shape == b.shape and np.abs(a - b).max(initial=0) <= 2


def test_oracle_post_on_replayed_tensors_equals_reference_results(replayed):
    """oracle/yolo_post.py and oracle/ufld_decode.py on the tensors HipEngine returned give the reference classes' results: the
    detections exactly (the head widened to float64 as the replay hands it over, integration_replay.py), the lane points within 1 px."""
    from oracle import yolo_post, ufld_decode
    got, fx = replayed
    lb = yolo_post.letterbox_params(fx["frame"].shape[:2], (640, 640))
    r = yolo_post.detect_post(fx["det_out0"][0].astype(np.float64), lb, "yolov8", 0.4, 0.45)
    d = got["det"]
    np.testing.assert_array_equal(np.asarray(r["xywh"], np.float64).reshape(-1, 4), np.asarray(d["xywh"], np.float64).reshape(-1, 4))
    np.testing.assert_array_equal(np.asarray(r["conf"], np.float64), np.asarray(d["conf"], np.float64))
    np.testing.assert_array_equal(np.asarray(r["xyxy_int"], np.int64).reshape(-1, 4), np.asarray(d["xyxy_int"], np.int64).reshape(-1, 4))
    labels = [str(s) for s in fx["labels"]]
    assert [labels[c] if c < len(labels) else "unknown" for c in np.asarray(r["class_id"]).tolist()] == d["label"]
    lanes, status = ufld_decode.process_output([fx["lane_out%d" % i] for i in range(4)], ufld_decode.ModelConfig("culane"),
                                               fx["frame"].shape[1], fx["frame"].shape[0])
    l = got["lane"]
    assert [bool(s) for s in status] == l["status"]
    for i in range(4):
        have = np.asarray(lanes[i], np.int64).reshape(-1, 2)
        want = np.asarray(l["points"][i], np.int64).reshape(-1, 2)
        assert have.shape == want.shape, (i, have.shape, want.shape)
        assert np.abs(have - want).max(initial=0) <= 1, (i, np.abs(have - want).max())
