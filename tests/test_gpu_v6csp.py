"""GPU: YOLOv6 v3.0 m / l (CSP-Bep networks, EffiDeHead with DFL).  The DFL decode kernel on the device's own predictor maps against a
float64 decode (including bin logits of |100|), both networks at 640 against the module-by-module oracle (tests/v6csp_oracle.py) in
every precision, the drop-in YoloDetector(model_type=YOLOV6) and one fused pipeline chain on m in the default precision, and a YOLOv6n
container still decoded by the 4-distance kernel."""
import importlib, os, tempfile

import numpy as np
import pytest

import netutil
import gpu_api
import parity_checks as pc
import chain_parity as CP
import v6csp_oracle as O
from conftest import load_pkg
from oracle import nets, preprocess, yolo_post

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
D = importlib.import_module("adas_amd.detectors")

TAPS = (("backbone.ERBlock_5.2.cv2.block.conv", "sppf"), ("neck.Rep_p3.cv3.block.conv", "p3"), ("neck.Rep_n3.cv3.block.conv", "p4"),
        ("neck.Rep_n4.cv3.block.conv", "p5"))


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b) + 1e-30))


def _kernels(e, batch):
    return {e.layer_kernel(i, batch) for i in range(e.stats()["num_layers"])}


@pytest.mark.parametrize("big", [False, True], ids=["synthetic", "logits100"])
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_dfl_decode_kernel(prec, big):
    """96x160 (levels 12x20, 6x10, 3x5: A = 315, not a multiple of the kernel's 32 rows), batch 3: the head against a float64 decode of the
    device's own reg_preds / cls_preds maps.  logits100: reg_preds scaled so bin logits reach |100| (expf overflows without the max)."""
    batch, hw = 3, (96, 160)
    ws = M.SynthWeights(0, gain=M.synth_gain("yolov6m"))
    M.build("yolov6m", wsrc=ws, imgsz=hw)
    W = dict(ws.store)
    x = netutil.coco_like_frames(batch, *hw, seed=5)
    path = os.path.join(tempfile.gettempdir(), f"v6m_dfl_{prec}_{int(big)}.hipm")
    if big:
        for i in range(3):
            w, b = W[f"detect.reg_preds.{i}.weight"], W[f"detect.reg_preds.{i}.bias"]
            W[f"detect.reg_preds.{i}.weight"] = (w * 40.0).astype(np.float32)
            W[f"detect.reg_preds.{i}.bias"] = (b + np.linspace(-60, 60, b.size)).astype(np.float32)
    g = M.build("yolov6m", wsrc=M.DictWeights(W), imgsz=hw)
    g.save(path)
    e = CE.HipEngine(path, prec, batch)
    got = np.array(e.engine_inference(x)[0], copy=True)
    regs = [e.fetch_activation(f"detect.reg_preds.{i}", batch) for i in range(3)]
    clss = [e.fetch_activation(f"detect.cls_preds.{i}", batch) for i in range(3)]
    kernels = _kernels(e, batch)
    e.close(); os.remove(path)
    assert got.shape == (batch, 315, 85)
    zmax = max(float(np.abs(r).max()) for r in regs)
    want = O.decode_np64(regs, clss, g.meta["strides"])
    eb, ep = float(np.abs(got[..., :4] - want[..., :4]).max()), float(np.abs(got[..., 4:] - want[..., 4:]).max())
    print("dfl %s %s: max|logit| %.1f  box max|diff| %.2e px  prob max|diff| %.2e" % (prec, "big" if big else "synth", zmax, eb, ep))
    assert "detect_v6_dfl_kernel" in kernels and "detect_v6_kernel" not in kernels, kernels
    assert zmax >= (100.0 if big else 1.0)
    assert np.all(np.isfinite(got)) and eb <= 1e-3 and ep <= 1e-6
    assert np.all(got[..., 4] == 1.0)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16", "fp16x3"])
@pytest.mark.parametrize("scale", ["m", "l"])
def test_yolov6_csp_640_vs_oracle(tmp_path, scale, prec):
    import bench
    name = "yolov6" + scale
    x = netutil.coco_like_frames(2, seed=11)
    path, W, g = bench.build_detector(M, CE, name, x, str(tmp_path), "v6c_" + prec, target_per_frame=100.0)
    taps = {}
    want = O.forward(x, W, scale, taps=taps)
    e = CE.HipEngine(path, precision=prec, max_batch=2)
    assert e.get_engine_output_shape()[0] == [[1, 8400, 85]]
    got = np.array(e.engine_inference(x)[0], copy=True)
    rtol = {"fp16": 5e-3, "bf16": 4e-2}
    for lname, key in TAPS:
        a = e.fetch_activation(lname, 2)
        ref = taps[key].numpy()
        err, rel = float(np.abs(a - ref).max()), rel_l2(a, ref)
        print("%s %s %-5s max|diff| %.3e  rel_l2 %.3e  max|ref| %.2f" % (name, prec, key, err, rel, np.abs(ref).max()))
        if prec in ("fp32", "fp16x3"):
            assert err <= 1e-3 * max(1.0, float(np.abs(ref).max())) and (prec == "fp32" or rel <= 1e-5), lname
        else:
            assert rel <= rtol[prec], lname
    ecls = float(np.abs(got[..., 4:] - want[..., 4:]).max())
    atol, rtol_b = {"fp32": (1e-3, 1e-5), "fp16": (0.1, 1e-2), "bf16": (1.0, 8e-2), "fp16x3": (1e-3, 1e-5)}[prec]
    ebox = float((np.abs(got[..., :4] - want[..., :4]) / (atol + rtol_b * np.abs(want[..., :4]))).max())
    n_over = int((want[..., 5:].max(axis=-1) > 0.4).sum())
    print("%s %s head: max|prob diff| %.3e  box %.3f of its bound  (%d anchors over 0.4)" % (name, prec, ecls, ebox, n_over))
    assert n_over >= 50 and np.all(got[..., 4] == 1.0)
    assert ecls <= {"fp32": 1e-4, "fp16": 2e-2, "bf16": 1.5e-1, "fp16x3": 1e-4}[prec] and ebox <= 1.0
    kernels = _kernels(e, 2)
    assert "detect_v6_dfl_kernel" in kernels and "depth2space_kernel" in kernels and "wsum_kernel" in kernels, kernels
    if prec == "fp16x3":
        netutil.assert_x3_convs(e, 2)
    e.close()
    if prec == "fp16x3":
        e = CE.HipEngine(path, max_batch=2)                    # no precision=: the default mode
        assert e.precision == "fp16x3"
        assert np.array_equal(np.asarray(e.engine_inference(x)[0]), got)
        e.close()


class _CspOracleChain(CP.OracleChain):
    """The oracle chain with the YOLOv6 m / l forward of tests/v6csp_oracle.py in place of oracle.nets.detector_forward."""

    def _forward(self, fn, *a, **k):
        if fn is nets.detector_forward:
            name, x, W = a[:3]
            return O.forward(x, W, name[len("yolov6"):])
        return super()._forward(fn, *a, **k)


def test_yolov6m_detector_dropin_and_pipeline_chain(tmp_path):
    """YoloDetector(model_type=YOLOV6) on m with no precision= (fp16x3) against the oracle head through oracle.yolo_post, and the fused
    pipeline (HEAD_V5 post-processing) against the oracle chain."""
    import bench
    cams = bench.cam_frames(4, 80)
    seam = np.concatenate([preprocess.yolo_prepare_input(f, (640, 640)) for f in cams])
    path, W, g = bench.build_detector(M, CE, "yolov6m", seam, str(tmp_path), "v6md", target_per_frame=80.0, capacity=1024)
    lab = tmp_path / "coco_label.txt"
    lab.write_text("\n".join(f"class{i}" for i in range(80)))
    det = D.YoloDetector(model_path=path, model_type=D.ObjectModelType.YOLOV6, classes_path=str(lab), box_score=0.4, box_nms_iou=0.45)
    eng = CE.OnnxEngine(path)
    assert det.engine.precision == eng.precision == "fp16x3"
    lb = yolo_post.letterbox_params((720, 1280), (640, 640))
    n_box = 0
    for f in cams[:2]:
        det.DetectFrame(f)
        x = preprocess.yolo_prepare_input(f, (640, 640))
        pc.check_yolo(det._last, yolo_post.detect_post(eng.engine_inference(x)[0][0], lb, "yolov5", 0.4, 0.45))   # its own head: bit-exact
        want = yolo_post.detect_post(O.forward(x, W, "m")[0], lb, "yolov5", 0.4, 0.45)                            # the oracle head
        got = det._last
        for k in ("cand_anchor", "cand_cls", "keep", "class_id"):
            np.testing.assert_array_equal(got[k], want[k])
        np.testing.assert_allclose(got["conf"], want["conf"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(got["xywh"], want["xywh"], rtol=1e-5, atol=1e-3)
        assert np.abs(np.asarray(got["xyxy_int"], np.int64) - np.asarray(want["xyxy_int"], np.int64)).max(initial=0) <= 1
        n_box += len(want["conf"])
    assert n_box > 0
    det.close(); eng.close()
    lane_path, Wl, gl = netutil.model("ufldv2_res18")
    pool = [cams[:2], cams[2:]]
    pipe = PL.AdasPipeline(path, lane_path, n_streams=2, src_hw=(720, 1280), head_layout=L.HEAD_V5, use_graph=True, max_candidates=1024)
    assert pipe.det.precision == "fp16x3"
    d_pool = [L.DeviceBuffer.from_array(np.ascontiguousarray(p)) for p in pool]
    chain = _CspOracleChain("yolov6m", W, "ufldv2_res18", Wl)
    st = CP.run_device_chain(pipe, lambda s: PP.YoloPost.fetch(pipe.post, s), lambda s: gpu_api.track_snapshot(*pipe.tracker.fetch(s)),
                             d_pool, pool, chain, 4, 2, [0, 1])
    pipe.close()
    for b in d_pool:
        b.free()
    o = st.summary()
    print("yolov6m pipeline default:", o)
    n = o["frames"]
    assert o["identical_candidate_sets"] == n and o["identical_survivors"] == n and o["identical_track_ids"] == o["track_states_compared"]
    assert o["lanes_within_1px"] == n and o["survivors_compared"] >= n


def test_yolov6n_container_keeps_4_distance_decode(tmp_path):
    """A container written before the DFL decode (params[5] = 0) loads and runs on detect_v6_kernel, its head unchanged."""
    path, W, g = netutil.model("yolov6n")
    assert [o for o in g.ops if o["type"] == M.OP_DETECT_V6][0]["params"][5:] == []
    x = netutil.coco_like_frames(2, seed=12)
    e = CE.HipEngine(path, "fp32", 2)
    got = np.array(e.engine_inference(x)[0], copy=True)
    kernels = _kernels(e, 2)
    e.close()
    assert "detect_v6_kernel" in kernels and "detect_v6_dfl_kernel" not in kernels, kernels
    want = nets.yolov6_forward(x, W, "n")
    assert float(np.abs(got[..., 4:] - want[..., 4:]).max()) <= 1e-3
    assert float((np.abs(got[..., :4] - want[..., :4]) / (1e-3 + 1e-5 * np.abs(want[..., :4]))).max()) <= 1.0


@pytest.mark.parametrize("reg_max", [16, 8])
def test_detect_v6_reg_max_mismatch_refused(tmp_path, reg_max):
    """A Detect op whose reg_max does not match its regression inputs (or is not 0 / 16) is refused at load, with the reason."""
    g = M.build("yolov6n", imgsz=(96, 160))
    op = [o for o in g.ops if o["type"] == M.OP_DETECT_V6][0]
    op["params"] = op["params"][:5] + [reg_max]
    path = g.save(str(tmp_path / "bad.hipm"))
    with pytest.raises(RuntimeError, match="reg_max"):          # _lib.AdasError (the package may be loaded under two module names)
        CE.HipEngine(path, "fp32", 1)
