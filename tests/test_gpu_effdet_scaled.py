"""GPU: EfficientDet-D1 / D2 / D3 and the two-pass tail.

  * the networks at their native sizes (640 / 768 / 896), batch 2, on camera-like frames against tests/effdet_oracle.py: C3 / C4 / C5 and
    the ten head tensors, in fp32, fp16x3 and fp16;
  * the tail (class-max pass over anchor chunks x frames, finish pass per frame) against oracle/effdet_tail.py at the native sizes and a
    non-square one, against the single-workgroup tail (ADAS_EFFDET_TAIL_ONE_WG=1 at create time) on the same device buffers -- synthetic
    heads and the D3 engine's own --, and its overflow report;
  * EfficientdetDetector on a D1 and a D3 container, 720p frames, against the oracle chain.
"""
import importlib
import os

import numpy as np
import pytest

import effdet_oracle as EO
import netutil
from conftest import load_pkg
from oracle import nets, effdet_tail, effdet_post, yolo_post

import test_gpu_configs as TG
from test_hostemu_logic import _effdet_heads

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PP = importlib.import_module("adas_amd.postproc")
D = importlib.import_module("adas_amd.detectors")

ONE_WG = "ADAS_EFFDET_TAIL_ONE_WG"


def _frames(n, seed):
    import bench
    return bench.cam_frames(n, seed)


@pytest.mark.parametrize("prec", ["fp32", "fp16x3", "fp16"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_efficientdet_scaled_vs_oracle(n, prec):
    """efficientdet-d<n> at its native size, batch 2: backbone features C3 / C4 / C5 and the ten head tensors against the torch oracle.
    fp32 / fp16x3: <= 1e-3 x max(1, |tensor| max) (the bound of test_efficientdet_d0_512_vs_oracle).
    fp16: rel-L2 <= twice the yardstick = the rel-L2 between the oracle and the same oracle with the weights and every stored activation
    rounded to half (oracle.nets.EMULATE = "fp16"), computed here on the same frames.  Yardstick values on these frames (CPU run):
                 c3        c4        c5        regression  class logits
        D1   1.474e-3  9.958e-4  6.577e-4   1.234e-3    3.845e-5
        D2   1.347e-3  8.163e-4  5.886e-4   7.322e-4    2.946e-5
        D3   1.024e-3  1.136e-3  8.917e-4   8.327e-4    3.014e-5
    (the class logits sit on the header bias, -4.2 / -4.0 / -3.42, which no rounding moves: their relative figure is small)."""
    name = "efficientdet-d%d" % n
    path, W, g = netutil.model(name)
    c = EO.config(n)
    S = c["imgsz"]
    assert (g.in_h, g.in_w) == (S, S) and len(g.outs) == 10
    x = np.concatenate([effdet_post.prepare_input(f, (S, S)) for f in _frames(2, 77)]).astype(np.float32)
    taps = {}
    reg, cls = EO.forward(x, W, c["stages"], c["fpn_c"], c["fpn_cells"], c["head_layers"], taps=taps)
    reg, cls = reg.numpy(), cls.numpy()
    want = dict(taps, regression=reg, classification=cls)
    yard = {}
    if prec == "fp16":
        nets.EMULATE = "fp16"
        try:
            t16 = {}
            r16, c16 = EO.forward(x, W, c["stages"], c["fpn_c"], c["fpn_cells"], c["head_layers"], taps=t16)
        finally:
            nets.EMULATE = None
        t16.update(regression=r16.numpy(), classification=c16.numpy())
        yard = {k: TG.rel_l2(t16[k], want[k]) for k in want}
    e = CE.HipEngine(path, precision=prec, max_batch=2)
    outs = e.engine_inference(x)
    got = {k: e.fetch_activation("blocks.%d.project" % b, 2) for k, b in zip(("c3", "c4", "c5"), EO.tap_blocks(c["stages"]))}
    e.close()
    rows = 9 * sum((S >> l) ** 2 for l in range(3, 8))
    got["regression"] = np.concatenate([o.reshape(2, -1, 4) for o in outs[0::2]], 1)
    got["classification"] = np.concatenate([o.reshape(2, -1, 90) for o in outs[1::2]], 1)
    assert got["regression"].shape == reg.shape == (2, rows, 4) and got["classification"].shape == cls.shape == (2, rows, 90)
    fails = []
    for key in ("c3", "c4", "c5", "regression", "classification"):
        err, rel = TG.report("%s %s %s" % (name, prec, key), got[key], want[key])
        if prec == "fp16":
            print("    yardstick %.3e, bound %.3e, measured %.3e" % (yard[key], 2 * yard[key], rel))
            if not rel <= 2 * yard[key]:
                fails.append((key, rel, 2 * yard[key]))
        else:
            bound = 1e-3 * max(1.0, float(np.abs(want[key]).max()))
            if not err <= bound:
                fails.append((key, err, bound))
    assert not fails, fails


def _upload(reg, cls, in_hw):
    rows = [9 * (in_hw[0] >> l) * (in_hw[1] >> l) for l in range(3, 8)]
    offs = np.concatenate([[0], np.cumsum(rows)])
    bufs_r = [L.DeviceBuffer.from_array(np.ascontiguousarray(reg[:, offs[l]:offs[l + 1]])) for l in range(5)]
    bufs_c = [L.DeviceBuffer.from_array(np.ascontiguousarray(cls[:, offs[l]:offs[l + 1]])) for l in range(5)]
    return bufs_r, bufs_c


def _tail_on(reg_ptrs, cls_ptrs, B, nc, in_hw, thr, iou, max_det, cap, one_wg):
    """Per-frame results of the device tail on device-resident level tensors; one_wg: the single-workgroup launch (switch read at create)."""
    old = os.environ.pop(ONE_WG, None)
    if one_wg:
        os.environ[ONE_WG] = "1"
    try:
        t = PP.EffdetTail(in_hw, nc, thr, iou, max_det, cap, B)
    finally:
        os.environ.pop(ONE_WG, None)
        if old is not None:
            os.environ[ONE_WG] = old
    try:
        t.run(reg_ptrs, cls_ptrs, B)
        return [t.fetch(b) for b in range(B)]
    finally:
        t.close()


def _same(a, b):
    assert a["n_candidates"] == b["n_candidates"]
    np.testing.assert_array_equal(a["class_id"], b["class_id"])
    np.testing.assert_array_equal(a["conf"], b["conf"])
    np.testing.assert_array_equal(a["boxes"], b["boxes"])


@pytest.mark.parametrize("seed,in_hw", [(0, (640, 640)), (1, (768, 768)), (2, (896, 896)), (3, (384, 640))], ids=lambda v: str(v))
def test_effdet_tail_two_pass_device_vs_oracle(seed, in_hw):
    """Batch 3, default launch (class-max pass + finish pass) against the numpy restatement: candidates, class ids, confidences and boxes
    identical; and against the single-workgroup launch on the same device buffers: identical arrays."""
    heads = [_effdet_heads(seed * 10 + b, in_hw) for b in range(3)]
    reg = np.stack([h[0] for h in heads]); cls = np.stack([h[1] for h in heads])
    bufs_r, bufs_c = _upload(reg, cls, in_hw)
    try:
        rp, cp = [b.ptr for b in bufs_r], [b.ptr for b in bufs_c]
        got = _tail_on(rp, cp, 3, 90, in_hw, 0.05, 0.5, 100, 3072, False)
        old = _tail_on(rp, cp, 3, 90, in_hw, 0.05, 0.5, 100, 3072, True)
    finally:
        for b in bufs_r + bufs_c:
            b.free()
    for b in range(3):
        want = effdet_tail.tail(reg[b], cls[b], in_hw, 0.05, 0.5, 100)
        print("tail %s frame %d: %d candidates -> %d kept" % (in_hw, b, want["n_candidates"], len(want["conf"])))
        assert want["n_candidates"] >= 100 and len(want["conf"]) >= 5
        _same(got[b], want)
        _same(got[b], old[b])


def test_effdet_tail_two_pass_equals_single_workgroup_on_d3_heads():
    """The D3 engine's own head tensors (fp16x3, two camera-like frames), read where the engine left them: both launches give identical arrays,
    at the engine's thresholds and at a score threshold of 0.048 (CPU run of the oracle: 1430 and 343 candidates)."""
    path, W, g = netutil.model("efficientdet-d3")
    x = np.concatenate([effdet_post.prepare_input(f, (896, 896)) for f in _frames(3, 5)[:2]]).astype(np.float32)
    e = CE.HipEngine(path, precision="fp16x3", max_batch=2)
    try:
        xb = L.DeviceBuffer.from_array(x)
        e.infer_device(xb.ptr, 2)
        rp = [e.output_device_ptr(2 * l) for l in range(5)]; cp = [e.output_device_ptr(2 * l + 1) for l in range(5)]
        n_seen = 0
        for thr, cap in ((0.05, 2048), (0.048, 3072)):
            new = _tail_on(rp, cp, 2, 90, (896, 896), thr, 0.5, 100, cap, False)
            old = _tail_on(rp, cp, 2, 90, (896, 896), thr, 0.5, 100, cap, True)
            for b in range(2):
                print("D3 heads, score_thr %.4f frame %d: %d candidates -> %d kept" % (thr, b, old[b]["n_candidates"], len(old[b]["conf"])))
                _same(new[b], old[b])
                n_seen += len(old[b]["conf"])
        assert n_seen >= 50
        xb.free()
    finally:
        e.close()


def test_effdet_tail_two_pass_overflow_fails_loudly():
    reg, cls = _effdet_heads(5, (128, 128), bias=0.0)
    bufs_r, bufs_c = _upload(reg[None], cls[None], (128, 128))
    try:
        for one_wg in (False, True):
            # the package may be loaded under two module names in one session, so the error is matched by text and code, not by class
            with pytest.raises(Exception, match="anchors over score_thr, max_candidates is 64") as ei:
                _tail_on([b.ptr for b in bufs_r], [b.ptr for b in bufs_c], 1, 90, (128, 128), 0.05, 0.5, 50, 64, one_wg)
            assert ei.value.code == -5      # ADAS_ERR_CAPACITY (include/adas_hip.h)
    finally:
        for b in bufs_r + bufs_c:
            b.free()


# (scale, box_score): the threshold sits in a gap of the oracle chain's confidences on these frames (CPU run: D1 0.0786 | 0.0961 on the
# last frame, every other detection of the second frame over 0.3; D3 0.052747 | 0.053009 on the third frame), 1e-4 and more away from
# any of them, so that the network's 1e-5 deviation cannot move a detection across it.
@pytest.mark.parametrize("n,thr", [(1, 0.085), (3, 0.0529)])
def test_efficientdet_scaled_detector_end_to_end(tmp_path, n, thr):
    """EfficientdetDetector(model_path=<efficientdet-d1 | -d3 container>), fp16x3: DetectFrame on 720p camera-like frames, compared as
    test_efficientdet_detector_end_to_end does:
    (a) the RectInfo list == the oracle's tail + __process_output restatement applied to the ENGINE's own head tensors;
    (b) == the oracle chain (torch network -> tail -> process_output): same count, labels, confidences within 1e-5, boxes within 0.01 px."""
    name = "efficientdet-d%d" % n
    path, W, g = netutil.model(name)
    c = EO.config(n)
    S = c["imgsz"]
    lab = tmp_path / "coco90.txt"
    lab.write_text("\n".join("c%d" % i for i in range(90)))
    det = D.EfficientdetDetector(model_path=path, classes_path=str(lab), box_score=thr, precision="fp16x3")
    assert det.engine.get_engine_output_shape()[1] == ["boxes", "class_ids", "scores"] and det.input_shapes == [1, 3, S, S]
    raw = CE.HipEngine(path, precision="fp16x3", max_batch=1)
    n_total = n_cand = 0
    for f in list(_frames(2, 78)) + list(_frames(3, 5)):
        det.DetectFrame(f)
        x = effdet_post.prepare_input(f, (S, S)).astype(np.float32)
        outs = raw.engine_inference(x)
        reg = np.concatenate([o.reshape(-1, 4) for o in outs[0::2]]); cls = np.concatenate([o.reshape(-1, 90) for o in outs[1::2]])
        lb = yolo_post.letterbox_params(f.shape[:2], (S, S))
        t = effdet_tail.tail(reg, cls, (S, S))
        assert det.engine.last_candidates[0] == t["n_candidates"] <= 2048
        n_cand += t["n_candidates"]
        want = effdet_post.process_output(t["boxes"], t["class_id"], t["conf"], lb, thr)
        info = det.object_info
        assert len(info) == len(want["conf"])
        for r, xywh, conf, cid in zip(info, want["xywh"], want["conf"], want["class_id"]):
            assert r.label == "c%d" % cid and r.conf == conf
            np.testing.assert_allclose([r.x, r.y, r.width, r.height], xywh, rtol=0, atol=2e-4)
        oreg, ocls = EO.forward(x, W, c["stages"], c["fpn_c"], c["fpn_cells"], c["head_layers"])
        to = effdet_tail.tail(oreg[0].numpy(), ocls[0].numpy(), (S, S))
        wo = effdet_post.process_output(to["boxes"], to["class_id"], to["conf"], lb, thr)
        print("%s frame: %d candidates (oracle %d), %d boxes over %.4f (oracle %d)" % (name, t["n_candidates"], to["n_candidates"], len(info), thr, len(wo["conf"])))
        assert all(abs(float(v) - thr) >= 1e-4 for v in to["conf"]), "the threshold must sit in a gap of the oracle's confidences"
        assert len(wo["conf"]) == len(info), (len(wo["conf"]), len(info))
        for r, xywh, conf, cid in zip(info, wo["xywh"], wo["conf"], wo["class_id"]):
            assert r.label == "c%d" % cid and abs(float(r.conf) - float(conf)) <= 1e-5
            np.testing.assert_allclose([r.x, r.y, r.width, r.height], xywh, rtol=0, atol=1e-2)
        n_total += len(info)
    print("%s detector fp16x3: %d candidates, %d boxes over %.4f on 5 frames" % (name, n_cand, n_total, thr))
    assert n_total >= 1
    raw.close(); det.close()
