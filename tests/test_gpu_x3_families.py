"""GPU: the split precision ("fp16x3", what `OnnxEngine(path)` runs) on the paths that only the YOLOv5 / v6 / v7 / v9 and UFLD families
reach, both sides of the thresholds its dispatcher selects kernels by, tensors at the 31-bit offset limit of the fused C2f launch, and the
default-precision fallback contract of coreEngine.HipEngine.

Every case is held to a plain higher-precision reference: torch on the device's own fetched inputs for single ops (max-pool and
upsample bit-exact, the rest at f32 class), the torch fp32 oracle of oracle/nets.py for whole networks.  Kernel labels are the strings
adas_engine_layer_kernel reports (bench.py groups its per-kernel table by them)."""
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import netutil
import test_gpu_conv as TC
from conftest import load_pkg
from oracle import nets

pytestmark = pytest.mark.gpu
load_pkg()
M = importlib.import_module("adas_amd.models")
CE = importlib.import_module("adas_amd.coreEngine")

X3_REL = 3e-6      # rel-L2 of one layer of the split precision against torch (tests/test_gpu_x3.py)
HERE = os.path.dirname(os.path.abspath(__file__))


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / (np.linalg.norm(b) + 1e-30))


def _save(g, d, tag):
    path = os.path.join(str(d), "%s.hipm" % tag)
    g.save(path)
    return path


def _run_case_in_child(env, H, W, cin, cout, k, s, act, batch):
    """TC.run_case in a fresh process: the kernel switches are read once per process."""
    code = ("import sys, json, importlib; sys.path.insert(0, %r); sys.path.insert(0, %r); from conftest import load_pkg; load_pkg();"
            "import test_gpu_conv as TC; CE = importlib.import_module('adas_amd.coreEngine'); info = {};"
            "rel, mx = TC.run_case(CE, %d, %d, %d, %d, %d, %d, %d, 0, 'fp16x3', batch=%d, info=info); print(json.dumps([rel, mx, info.get('kernel')]))"
            % (os.path.dirname(HERE), HERE, H, W, cin, cout, k, s, act, batch))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


# ---------------------------------------------------------------------------------------------------------------------------- single ops

@pytest.mark.parametrize("k,s,p,c,hw", [(2, 2, 0, 32, (40, 56)), (2, 2, 0, 64, (23, 37)), (3, 2, 1, 64, (80, 400)), (3, 2, 1, 32, (23, 37)),
                                        (3, 1, 1, 96, (13, 17)), (5, 1, 2, 32, (20, 20)), (5, 1, 2, 64, (13, 17)), (9, 1, 4, 32, (20, 20)),
                                        (13, 1, 6, 40, (11, 9))], ids=str)
def test_maxpool_x3_bit_exact(tmp_path, k, s, p, c, hw):
    """maxpool_x3_kernel<2|3> (YOLOv7's MP, the ResNet stem pool) and the generic maxpool_kernel<x3s> (SPPF's 5x5, SPPCSPC's 9 / 13):
    a max selects one of its inputs and rounds nothing, so the output has to equal torch's max-pool of the fetched input bit for bit --
    on whole and ragged maps, windows cut by the image edge, channel counts of one to twelve G8 groups."""
    H, W = hw
    batch = 3
    g = M.Graph("mpunit", 3, H, W, M.SynthWeights(6, gain=1.0))
    x, c3 = g.input()
    a = g.conv(x, c, 1, 1, "expand", act=M.ACT_SILU, true_cin=c3)
    y = g.maxpool(a, k, s, p, name="test")
    z = g.conv(y, 8, 1, 1, "tap", act=M.ACT_NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    path = _save(g, tmp_path, "mp")
    e = CE.HipEngine(path, "fp16x3", batch)
    xin = np.random.default_rng(3).uniform(-1, 1, (batch, 3, H, W)).astype(np.float32)
    e.engine_inference(xin)
    got = e.fetch_activation("test", batch)
    a_dev = e.fetch_activation("expand", batch)
    label = e.layer_kernel(e.layer_index("test"), batch)
    e.close(); os.remove(path)
    want = F.max_pool2d(torch.from_numpy(a_dev).double(), k, s, p).float().numpy()
    assert label == "maxpool_kernel", label
    assert got.shape == want.shape
    n_bad = int((got != want).sum())
    assert n_bad == 0, (n_bad, float(np.abs(got - want).max()))


@pytest.mark.parametrize("hw", [(20, 20), (13, 23)], ids=str)
def test_upsample_x3_alone_and_folded_into_its_consumer(tmp_path, hw, monkeypatch):
    """YOLO necks: Upsample -> Concat -> 1x1 conv.  Folded (the default), conv_pwx3 reads the upsampled channels at (y / 2, x / 2) of the
    half-resolution tensor (ConvArgs::up) and the upsample launch is dropped: the conv against float64 torch on the fetched inputs.
    Unfolded (ADAS_NO_UPSAMPLE_FOLD=1, read when an engine is created), upsample2_kernel moves whole 32-byte G8 groups: bit-exact, and
    the conv behind it agrees with the folded one bit for bit (same values in, same arithmetic)."""
    H, W = hw
    batch = 3
    ws = M.SynthWeights(8, gain=1.0)
    g = M.Graph("upunit", 3, 2 * H, 2 * W, ws)
    x, c3 = g.input()
    lo = g.conv(x, 32, 3, 2, "down", act=M.ACT_SILU, true_cin=c3)
    cat = g.buf(2 * H, 2 * W, 64)
    g.upsample2(lo, out=cat.slice(0, 32), name="up")
    g.conv(x, 32, 1, 1, "side", act=M.ACT_SILU, true_cin=c3, out=cat.slice(32, 32))
    y = g.conv(cat, 48, 1, 1, "test", act=M.ACT_SILU)
    z = g.conv(y, 8, 1, 1, "tap", act=M.ACT_NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    path = _save(g, tmp_path, "up")
    xin = np.random.default_rng(2).uniform(0, 1, (batch, 3, 2 * H, 2 * W)).astype(np.float32)
    res = {}
    for folded in (True, False):
        if folded:
            monkeypatch.delenv("ADAS_NO_UPSAMPLE_FOLD", raising=False)
        else:
            monkeypatch.setenv("ADAS_NO_UPSAMPLE_FOLD", "1")
        e = CE.HipEngine(path, "fp16x3", batch)
        e.engine_inference(xin)
        labels = (e.layer_kernel(e.layer_index("up"), batch), e.layer_kernel(e.layer_index("test"), batch))
        res[folded] = dict(labels=labels, test=e.fetch_activation("test", batch), lo=e.fetch_activation("down", batch),
                           side=e.fetch_activation("side", batch), up=None if folded else e.fetch_activation("up", batch))
        e.close()
    os.remove(path)
    print("upsample x3 %s: folded %s, unfolded %s" % (hw, res[True]["labels"], res[False]["labels"]))
    assert res[True]["labels"][0] == "(folded into the consumer's loads)" and "conv_pwx3_kernel" in res[True]["labels"][1]
    assert res[False]["labels"][0] == "upsample2_kernel" and "conv_pwx3_kernel" in res[False]["labels"][1]
    r = res[False]
    assert np.array_equal(r["up"], np.repeat(np.repeat(r["lo"], 2, 2), 2, 3))
    assert np.array_equal(res[True]["lo"], r["lo"]) and np.array_equal(res[True]["side"], r["side"])
    Wt = {k_: torch.from_numpy(v).double() for k_, v in ws.store.items()}
    lo_, side_ = torch.from_numpy(res[True]["lo"]).double(), torch.from_numpy(res[True]["side"]).double()
    want = F.silu(F.conv2d(torch.cat([F.interpolate(lo_, scale_factor=2, mode="nearest"), side_], 1), Wt["test.weight"], Wt["test.bias"])).numpy()
    rel = rel_l2(res[True]["test"], want)
    print("upsample x3 %s: folded conv rel %.2e" % (hw, rel))
    assert rel < X3_REL, rel
    assert np.array_equal(res[True]["test"], r["test"])


@pytest.mark.parametrize("name,hw,nc", [("yolov7-tiny", (224, 352), 3), ("yolov5n", (160, 96), 80), ("yolov5s", (64, 64), 91)], ids=str)
def test_v5_layout_detect_on_x3_heads(name, hw, nc):
    """In the split precision the v5-layout Detect is not fused with its 1x1 convs (det5_applicable refuses it): the per-level convs run
    on x3 kernels with fp32 outputs and detect_v5_kernel decodes them.  The oracle's Detect on the activations the device fed those convs
    (fetched), with fp32 weights: every element of the (A, 5 + nc) head within 1e-4 (probabilities) / 1e-3 px + 1e-4 relative (boxes),
    in the oracle's (level, anchor, y, x) row order -- ragged level sizes, 3 frames, class counts other than 80."""
    path, W, g = netutil.model(name, imgsz=hw, nc=nc)
    x = netutil.coco_like_frames(3, hw[0], hw[1], seed=21)
    e = CE.HipEngine(path, precision="fp16x3", max_batch=3)
    got = e.engine_inference(x)[0]
    kernels = [e.layer_kernel(i, 3) for i in range(e.stats()["num_layers"])]
    det = [o for o in g.ops if o["type"] == M.OP_DETECT_V5][0]
    head_convs = [[o for o in g.ops if o["type"] == M.OP_CONV and o["out"].buf == v.buf][0] for v in det["ins"]]
    feeders = [[o for o in g.ops if o["type"] == M.OP_CONV and o["out"].buf == hc["ins"][0].buf and o["out"].coff == hc["ins"][0].coff][0] for hc in head_convs]
    feats = [torch.from_numpy(e.fetch_activation(f["name"], 3)) for f in feeders]
    head_labels = [e.layer_kernel(e.layer_index(hc["name"]), 3) for hc in head_convs]
    netutil.assert_x3_convs(e, 3)
    e.close()
    assert "detect_v5_kernel" in kernels and "detect_v5_fused_kernel" not in kernels, kernels
    assert all("x3" in k for k in head_labels), head_labels
    fmt = head_convs[0]["name"].rsplit(".", 1)[0] + ".{}"
    anchors = M.V7_TINY_ANCHORS if name.startswith("yolov7") else M.V5_ANCHORS
    want = nets._v5_decode(feats, W, fmt, nc, anchors, hw[0])
    assert got.shape == want.shape
    ecls = float(np.abs(got[..., 4:] - want[..., 4:]).max())
    ebox = float((np.abs(got[..., :4] - want[..., :4]) / (1e-3 + 1e-4 * np.abs(want[..., :4]))).max())
    print("%s %s fp16x3 nc=%d: max|prob diff| %.3e, box %.3f of its bound" % (name, hw, nc, ecls, ebox))
    assert ecls <= 1e-4 and ebox <= 1.0


def test_v6_detect_on_x3_heads():
    """YOLOv6's anchor-free Detect (detect_v6_kernel) fed by the split precision's per-level cls / reg 1x1 convs (fp32 outputs): the
    decode against float64 torch on the fetched head tensors, restating oracle.nets.yolov6_forward's tail (sigmoid class scores,
    (cx, cy, w, h) = distances around the cell centre x stride, objectness 1) -- a 224 x 352 input (levels 28 x 44, 14 x 22 and a ragged
    7 x 11), 3 classes, 3 frames, in the oracle's (level, y, x) row order: probabilities within 1e-4, boxes within 1e-3 px + 1e-4 relative."""
    nc, (H, W_) = 3, (224, 352)
    path, Wt, g = netutil.model("yolov6n", imgsz=(H, W_), nc=nc)
    x = netutil.coco_like_frames(3, H, W_, seed=23)
    e = CE.HipEngine(path, precision="fp16x3", max_batch=3)
    got = np.array(e.engine_inference(x)[0], copy=True)
    kernels = [e.layer_kernel(i, 3) for i in range(e.stats()["num_layers"])]
    netutil.assert_x3_convs(e, 3)
    cls = [torch.from_numpy(e.fetch_activation("detect.cls_preds.%d" % i, 3)).double() for i in range(3)]
    reg = [torch.from_numpy(e.fetch_activation("detect.reg_preds.%d" % i, 3)).double() for i in range(3)]
    e.close()
    assert "detect_v6_kernel" in kernels, kernels
    assert [tuple(c.shape[2:]) for c in cls] == [(28, 44), (14, 22), (7, 11)]
    cl, rg, pts, strd = [], [], [], []
    for c, r in zip(cls, reg):
        b, _, h, w = c.shape
        cl.append(torch.sigmoid(c).reshape(b, nc, h * w))
        rg.append(r.reshape(b, 4, h * w))
        sy, sx = torch.meshgrid(torch.arange(h, dtype=torch.float64) + 0.5, torch.arange(w, dtype=torch.float64) + 0.5, indexing="ij")
        pts.append(torch.stack((sx, sy), -1).reshape(-1, 2))
        strd.append(torch.full((h * w, 1), float(H // h), dtype=torch.float64))
    score, dist = torch.cat(cl, -1).permute(0, 2, 1), torch.cat(rg, -1).permute(0, 2, 1)
    ap, st = torch.cat(pts), torch.cat(strd)
    x1y1, x2y2 = ap - dist[..., :2], ap + dist[..., 2:]
    boxes = torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), -1) * st
    want = torch.cat((boxes, torch.ones(boxes.shape[0], boxes.shape[1], 1, dtype=torch.float64), score), -1).numpy()
    assert got.shape == want.shape == (3, 28 * 44 + 14 * 22 + 7 * 11, 5 + nc)
    ecls = float(np.abs(got[..., 4:] - want[..., 4:]).max())
    ebox = float((np.abs(got[..., :4] - want[..., :4]) / (1e-3 + 1e-4 * np.abs(want[..., :4]))).max())
    print("yolov6n 224x352 fp16x3 nc=3 Detect: max|prob diff| %.3e, box %.3f of its bound" % (ecls, ebox))
    assert ecls <= 1e-4 and ebox <= 1.0


# ------------------------------------------------------------------------------------------------------------- every family at batch 64

DETECTORS = ["yolov5n", "yolov5s", "yolov6n", "yolov6s", "yolov7-tiny", "yolov9t", "yolov9s", "yolov9c"]
LANES = {"ufld_v1_res18": (dict(), (288, 800)), "ufld_v1_culane_res18": (dict(), (288, 800)), "ufldv2_tusimple_res18": (dict(), (320, 800)),
         "ufldv2_curvelanes_res18": (dict(in_h=256, in_w=512), (256, 512))}


def _lane_oracle(name, x, W, g):
    if name.startswith("ufld_v1"):
        G, K = (200, 18) if "culane" in name else (100, 56)
        return [nets.ufld_v1_forward(x, W, "18", G, K)]
    if "tusimple" in name:
        return nets.ufldv2_forward(x, W, "18", 100, 56, 100, 41, fc_norm=False)
    return nets.ufldv2_forward(x, W, "18", 200, 72, 100, 41, num_lanes=10)


@pytest.mark.parametrize("name", DETECTORS + list(LANES))
def test_family_at_the_bench_batch_in_the_default_mode(name):
    """Each family at batch 64 (bench.py's stream count), opened with no precision= (the default: fp16x3).  Kernel selection differs from
    the small-batch tests: conv_h8x3, conv_s2d_x3 and conv_pwx3 take over from the small-map kernels.  Three distinct frames tiled over
    the batch: frames 0-2 against the torch fp32 oracle, every copy bit-identical to its original.  Lane outputs: max|diff| <= 1e-3 x
    max(1, max|ref|) and rel-L2 <= 1e-5.  Detector heads: boxes <= 1e-3 x max|box|, class probabilities <= 1e-4 and head rel-L2 <= 1e-4 --
    each raised only to 3x what the fp32 mode itself reaches on the same three frames where that is larger (these heads are not calibrated:
    a near-zero logit of a deep random-weight net moves with the summation order), and probabilities never above the fp32 legs' 1e-3."""
    B = 64
    lane = name in LANES
    if lane:
        kw, (h, w) = LANES[name]
        path, W, g = netutil.model(name, **kw)
        x3 = netutil.lane_frames(3, h, w, seed=13)
        want = _lane_oracle(name, x3, W, g)
    else:
        path, W, g = netutil.model(name)
        x3 = netutil.coco_like_frames(3, seed=13)
        want = [nets.detector_forward(name, x3, W)]
    x = np.ascontiguousarray(np.concatenate([x3] * 22, 0)[:B])
    e = CE.OnnxEngine(path, max_batch=B)
    assert e.precision == "fp16x3"
    labels = netutil.assert_x3_convs(e, B)
    print("%s batch %d kernels: %s" % (name, B, sorted({v.split("<")[0] for v in labels.values()})))
    got = e.engine_inference(x)
    e.close()
    if not lane:   # the fp32 mode on the same frames: the yardstick the split precision's head bounds may be raised to
        e32 = CE.HipEngine(path, precision="fp32", max_batch=3)
        h32 = e32.engine_inference(x3)[0]
        e32.close()
    for o, wv in zip(got, want):
        rel = rel_l2(o[:3], wv)
        if lane:
            err = float(np.abs(o[:3] - wv).max())
            print("%s batch %d fp16x3: max|diff| %.3e rel %.3e" % (name, B, err, rel))
            assert err <= 1e-3 * max(1.0, float(np.abs(wv).max())) and rel <= 1e-5
        else:
            v5 = o.shape[-1] == 5 + 80
            box = (lambda t: t[..., :4]) if v5 else (lambda t: t[:, :4])
            cls = (lambda t: t[..., 4:]) if v5 else (lambda t: t[:, 4:])
            ecls = float(np.abs(cls(o[:3]) - cls(wv)).max())
            ebox = float(np.abs(box(o[:3]) - box(wv)).max())
            rel32, ecls32 = rel_l2(h32, wv), float(np.abs(cls(h32) - cls(wv)).max())
            print("%s batch %d fp16x3: rel %.3e max|prob diff| %.3e max|box diff| %.3e px  (fp32 mode, 3 frames: rel %.3e max|prob diff| %.3e)"
                  % (name, B, rel, ecls, ebox, rel32, ecls32))
            assert rel <= max(1e-4, 3 * rel32) and ecls <= min(1e-3, max(1e-4, 3 * ecls32))
            assert ebox <= 1e-3 * max(1.0, float(np.abs(box(wv)).max()))
        for k in range(3, B):
            assert np.array_equal(o[k], o[k % 3]), (k, float(np.abs(o[k] - o[k % 3]).max()))


# ------------------------------------------------------------------------------------------------------------- selection thresholds
#
# conv_x3.hip, for a conv on the generic kernel (M = batch x Ho x Wo output pixels, K steps = kpad / 32, kpad = kh kw Cin rounded up to 32):
#   conv_x3_ksplit    when Cout >= 32, K steps >= 16 and ceil(M / 64) x ceil(Cout / 64) <= 128 (ADAS_X3_KSPLIT_TILES = 129);
#                     its 32 x 64 tiles when Cout >= 64 and ceil(M / 32) x ceil(Cout / 32) > 320 (ADAS_X3_KSPLIT_WIDE), else 32 x 32
#   conv_x3_igemm     otherwise: BN = 16 / 32 / 64 for Cout <= 16 / <= 32 / more; BM = 128 when ceil(M / 128) x ceil(Cout / BN) >= 512,
#                     else 64, 32 when (BN >= 32 and ceil(M / 64) x ceil(Cout / BN) < 128), then BN = 32 when (BN = 64 and
#                     ceil(M / 32) x ceil(Cout / 64) < 128)
# 1x1 convs with Cin = 480 or 544 (15 / 17 K steps of 32) are outside conv_pwx3's K-step set and land on the generic kernel.

def _cdiv(a, b):
    return -(-a // b)


def _ksplit_applies(M_, cout, ksteps):
    return cout >= 32 and ksteps >= 16 and _cdiv(M_, 64) * _cdiv(cout, 64) <= 128


def _ksplit_wide(M_, cout):
    return cout >= 64 and _cdiv(M_, 32) * _cdiv(cout, 32) > 320


def _igemm_tile(M_, cout):
    bn = 16 if cout <= 16 else (32 if cout <= 32 else 64)
    if _cdiv(M_, 128) * _cdiv(cout, bn) >= 512 and M_ > 64:
        return 128, bn
    bm = 64
    if bn >= 32:
        if _cdiv(M_, 64) * _cdiv(cout, bn) < 128:
            bm = 32
        if bm == 32 and bn == 64 and _cdiv(M_, 32) * _cdiv(cout, 64) < 128:
            bn = 32
    return bm, bn


# (H, W, Cout): 1x1, Cin 544 (17 K steps), batch 1
KSPLIT_WIDTH_CASES = [(40, 128, 64), (41, 125, 64), (53, 64, 80), (57, 61, 80), (53, 64, 96), (61, 67, 96), (45, 32, 200), (37, 43, 200)]


@pytest.mark.parametrize("case", KSPLIT_WIDTH_CASES, ids=str)
def test_ksplit_tile_width_threshold(case):
    """conv_x3_ksplit picks 32 x 64 tiles when its 32 x 32 grid would exceed 320 workgroups.  M = H x W at batch 1, Cin 544 (17 K steps):
      Cout  64: ceil(M / 32) x 2 > 320  <=>  M > 5120:  40 x 128 = 5120 -> 160 x 2 = 320 (32 x 32);  41 x 125 = 5125 -> 161 x 2 = 322 (32 x 64)
      Cout  80: ceil(M / 32) x 3 > 320  <=>  M > 3392:  53 x 64 = 3392 -> 106 x 3 = 318;  57 x 61 = 3477 -> 109 x 3 = 327
      Cout  96: the same 3 column tiles:                53 x 64 = 3392 -> 318;            61 x 67 = 4087 -> 128 x 3 = 384
      Cout 200: ceil(M / 32) x 7 > 320  <=>  M > 1440:  45 x 32 = 1440 -> 45 x 7 = 315;   37 x 43 = 1591 -> 50 x 7 = 350
    and every case stays on the K-split kernel: ceil(M / 64) x ceil(Cout / 64) <= 128 (81 x 1, 54 x 2, 64 x 2, 23 x 4 at the largest M).
    The label does not name the tile width, so the wide side also runs with ADAS_X3_KSPLIT_WIDE=100000 in a child process (the 32 x 32
    form of the same layer): both forms f32-class against torch, and the same bits on a second run (the reduction order is fixed)."""
    H, W, cout = case
    M_ = H * W
    assert _ksplit_applies(M_, cout, 17)
    wide = _ksplit_wide(M_, cout)
    assert wide == (case in KSPLIT_WIDTH_CASES[1::2]), (case, _cdiv(M_, 32) * _cdiv(cout, 32))
    info, run1, run2 = {}, {}, {}
    rel, mx = TC.run_case(CE, H, W, 544, cout, 1, 1, M.ACT_SILU, M.RES_NONE, "fp16x3", batch=1, info=info, keep=run1)
    print("x3 k-split width %s (%s): rel %.2e max %.2e  %s" % (case, "32x64" if wide else "32x32", rel, mx, info["kernel"]))
    assert "conv_x3_ksplit_kernel" in info["kernel"], info
    assert rel < X3_REL and mx < 1e-4, (case, rel, mx)
    TC.run_case(CE, H, W, 544, cout, 1, 1, M.ACT_SILU, M.RES_NONE, "fp16x3", batch=1, keep=run2)
    assert np.array_equal(run1["got"], run2["got"])
    if wide:
        rel2, mx2, kernel = _run_case_in_child({"ADAS_X3_KSPLIT_WIDE": "100000"}, H, W, 544, cout, 1, 1, M.ACT_SILU, 1)
        print("x3 k-split width %s forced 32x32: rel %.2e max %.2e  %s" % (case, rel2, mx2, kernel))
        assert "conv_x3_ksplit_kernel" in kernel and rel2 < X3_REL and mx2 < 1e-4, (rel2, mx2, kernel)


# (H, W, Cin, k, Cout, expected kernel)
KSPLIT_VS_IGEMM_CASES = [(64, 128, 544, 1, 64, "conv_x3_ksplit_kernel"), (65, 127, 544, 1, 64, "conv_x3_igemm_kernel<64,64>"),
                         (32, 127, 544, 1, 128, "conv_x3_ksplit_kernel"), (33, 125, 544, 1, 128, "conv_x3_igemm_kernel<64,64>"),
                         (10, 20, 480, 1, 64, "conv_x3_igemm_kernel<32,32>"), (10, 20, 56, 3, 64, "conv_x3_ksplit_kernel")]


@pytest.mark.parametrize("case", KSPLIT_VS_IGEMM_CASES, ids=str)
def test_ksplit_vs_igemm_threshold(case):
    """conv_x3_ksplit takes a launch whose 64 x 64 tiling is at most 128 workgroups and whose K loop is at least 16 steps of 32:
      Cout  64, Cin 544 (17 steps): 64 x 128 = 8192 px -> ceil(8192 / 64) x 1 = 128 (K-split);  65 x 127 = 8255 -> 129 x 1 = 129 (igemm,
                                    BM 64 as ceil(8255 / 64) x 1 = 129 >= 128, BN 64)
      Cout 128, Cin 544:            32 x 127 = 4064 -> 64 x 2 = 128;  33 x 125 = 4125 -> 65 x 2 = 130 (igemm <64,64>: 65 x 2 >= 128)
      K steps at 10 x 20 = 200 px, Cout 64 (4 x 1 = 4 tiles): 1x1 Cin 480 -> kpad 480 = 15 steps (igemm: ceil(200 / 64) x 1 = 4 < 128 ->
                                    BM 32, ceil(200 / 32) x 1 = 7 < 128 -> BN 32); 3x3 Cin 56 -> 9 x 56 = 504 -> kpad 512 = 16 steps (K-split)
    f32-class against torch on either side; the K-split side gives the same bits on a second run."""
    H, W, cin, k, cout, want_kernel = case
    M_ = H * W
    ks = _cdiv(k * k * cin, 32)
    on_ksplit = _ksplit_applies(M_, cout, ks)
    assert on_ksplit == (want_kernel == "conv_x3_ksplit_kernel"), (case, ks, _cdiv(M_, 64) * _cdiv(cout, 64))
    if not on_ksplit:
        assert want_kernel == "conv_x3_igemm_kernel<%d,%d>" % _igemm_tile(M_, cout)
    info, run1, run2 = {}, {}, {}
    rel, mx = TC.run_case(CE, H, W, cin, cout, k, 1, M.ACT_SILU, M.RES_NONE, "fp16x3", batch=1, info=info, keep=run1)
    print("x3 k-split / igemm %s: rel %.2e max %.2e  %s" % (case, rel, mx, info["kernel"]))
    assert info["kernel"] == want_kernel, info
    assert rel < X3_REL and mx < 1e-4, (case, rel, mx)
    if on_ksplit:
        TC.run_case(CE, H, W, cin, cout, k, 1, M.ACT_SILU, M.RES_NONE, "fp16x3", batch=1, keep=run2)
        assert np.array_equal(run1["got"], run2["got"])


# (H, W, Cout, batch, expected tile): 1x1, Cin 480 (15 K steps: never the K-split kernel)
IGEMM_TILE_CASES = [(256, 256, 16, 1, (128, 16)), (255, 256, 16, 1, (64, 16)), (64, 127, 32, 1, (32, 32)), (64, 128, 32, 1, (64, 32)),
                    (63, 64, 64, 1, (32, 32)), (64, 64, 64, 1, (32, 64)), (64, 128, 64, 1, (64, 64)), (128, 128, 64, 4, (128, 64))]


@pytest.mark.parametrize("case", IGEMM_TILE_CASES, ids=str)
def test_igemm_tile_shapes(case):
    """conv_x3_igemm's tile per launch (1x1, Cin 480 = 15 K steps, so never the K-split kernel):
      Cout 16 (BN 16): BM 128 when ceil(M / 128) >= 512:  256 x 256 = 65536 -> 512 (<128,16>);  255 x 256 = 65280 -> 510 (<64,16>)
      Cout 32 (BN 32): BM 32 when ceil(M / 64) < 128:     64 x 127 = 8128 -> 127 (<32,32>);     64 x 128 = 8192 -> 128 (<64,32>)
      Cout 64 (BN 64): 63 x 64 = 4032 -> ceil(M / 64) = 63 < 128 -> BM 32, ceil(M / 32) = 126 < 128 -> BN 32 (<32,32>);
                       64 x 64 = 4096 -> 64 < 128 -> BM 32, 128 -> BN stays 64 (<32,64>);  64 x 128 = 8192 -> 128 (<64,64>);
                       4 x 128 x 128 = 65536 -> ceil(M / 128) = 512 (<128,64>)
    every one f32-class against torch (ragged M and a batch of 4 included)."""
    H, W, cout, batch, tile = case
    assert _igemm_tile(batch * H * W, cout) == tile and not _ksplit_applies(batch * H * W, cout, 15)
    info = {}
    rel, mx = TC.run_case(CE, H, W, 480, cout, 1, 1, M.ACT_SILU, M.RES_NONE, "fp16x3", batch=batch, info=info)
    print("x3 igemm tile %s: rel %.2e max %.2e  %s" % (case, rel, mx, info["kernel"]))
    assert info["kernel"] == "conv_x3_igemm_kernel<%d,%d>" % tile, info
    assert rel < X3_REL and mx < 1e-4, (case, rel, mx)


@pytest.mark.parametrize("batch", [95, 96])
def test_stride2_kernel_item_floor(batch):
    """The stride-2 kernels of the split precision launch from 96 items (ADAS_S2X_MIN_ITEMS): a 32 x 32 -> 16 x 16 map, Cin 32 -> Cout 64,
    is one item per frame (plan_s2, S2_BM = 256: strip width 16 fills its tiles completely, NS = 1, TPS = ceil(16 x 16 / 256) = 1, one
    64-channel block), so 95 frames = 95 items stay on conv_x3_igemm and 96 frames = 96 items take conv_s2d_x3 -- the whole batch
    f32-class against torch on both sides."""
    info = {}
    rel, mx = TC.run_case(CE, 32, 32, 32, 64, 3, 2, M.ACT_SILU, M.RES_NONE, "fp16x3", batch=batch, info=info)
    print("x3 stride 2 at %d items: rel %.2e max %.2e  %s" % (batch, rel, mx, info["kernel"]))
    assert ("conv_s2d_x3_kernel" if batch >= 96 else "conv_x3_igemm_kernel") in info["kernel"], info
    assert rel < X3_REL and mx < 1e-4, (batch, rel, mx)


@pytest.mark.parametrize("batch,act", [(16, M.ACT_LEAKY), (64, M.ACT_LEAKY)])
def test_leaky_relu_on_the_batch_64_x3_kernels(batch, act):
    """yolov7-tiny's layer shapes with LeakyReLU(0.1) in the split precision at the pipeline's stream counts: the persistent kernels
    (conv_h8x3 for the 3x3 stride-1 layers, conv_s2d_x3 for the stride-2 ones) and conv_pwx3, f32-class against torch."""
    seen = set()
    for cin, cout, k, s, (H, W) in [(32, 32, 3, 1, (160, 160)), (64, 64, 3, 1, (80, 80)), (128, 128, 3, 1, (40, 40)), (256, 512, 3, 1, (20, 20)),
                                    (64, 128, 3, 2, (80, 80)), (128, 256, 3, 2, (80, 80)), (128, 64, 1, 1, (80, 80))]:
        info = {}
        rel, mx = TC.run_case(CE, H, W, cin, cout, k, s, act, M.RES_NONE, "fp16x3", batch=batch, info=info)
        print("leaky x3 b%d %s -> %s  rel %.2e max %.2e" % (batch, (cin, cout, k, s, H, W), info["kernel"], rel, mx))
        assert "x3" in info["kernel"] and rel < X3_REL and mx < 1e-4, (cin, cout, k, s, info, rel, mx)
        seen.add(info["kernel"].split("<")[0])
    if batch == 64:
        assert {"conv_h8x3_kernel", "conv_s2d_x3_kernel"} <= seen, seen


# (batch, on conv_h8x3): 3x3 64 -> 64 on a 16 x 16 map, one X8_BM = 256-pixel tile per frame
H8_FILL_CASES = [(88, False), (89, True), (248, True), (304, False), (305, True)]


@pytest.mark.parametrize("batch,h8", H8_FILL_CASES, ids=str)
def test_h8x3_acceptance_thresholds(batch, h8):
    """conv_h8x3 takes a launch (x8_blocks_per_unit, X8_SLOTS = 32 workgroup slots per XCD) when its units per XCD fill the last round to
    at least 0.6 (ADAS_H8X_MIN_FILL), or number 12-31 (one partial round).  A 16 x 16 map is one 256-pixel tile per frame (x8_plan: strip
    width 16, 16 rows, NS = TPS = 1) and Cout 64 is one block, so units = ceil(batch / 8):
      batch  88 -> 11 units: under 32 and under 12              -> conv_x3_igemm
      batch  89 -> 12 units: the 12-31 branch                   -> conv_h8x3
      batch 248 -> 31 units: the 12-31 branch                   -> conv_h8x3
      batch 304 -> 38 units: 2 rounds, 38 / 64 = 0.594 < 0.6    -> conv_x3_igemm
      batch 305 -> 39 units: 2 rounds, 39 / 64 = 0.609 >= 0.6   -> conv_h8x3
    The last frame (the highest offsets) f32-class against torch on every side."""
    info = {}
    rel, mx = _run_last_frame(16, 16, 64, 64, 1, batch, info)
    print("h8x3 acceptance at %d frames (%d units): last frame rel %.2e max %.2e  %s" % (batch, -(-batch // 8), rel, mx, info["kernel"]))
    assert ("conv_h8x3_kernel" if h8 else "conv_x3_igemm_kernel") in info["kernel"], info
    assert rel < X3_REL and mx < 1e-4, (batch, rel, mx)


# ------------------------------------------------------------------------------------------------------------- 31-bit offsets

@pytest.mark.parametrize("max_batch,fused", [(40, True), (48, False)])
def test_c2f_fusion_at_the_31_bit_input_limit(tmp_path, max_batch, fused):
    """conv_c2f_x3.hip addresses the block input with 31-bit byte offsets at 4 bytes per element and refuses a launch that reaches 2^31
    bytes.  The fusion is decided when the engine is created, at max_batch: a 32-channel input at 640 x 640 is
      max_batch 40: 40 x 640 x 640 x 32 x 4 = 2.10e9 < 2^31 = 2.147e9 -> fused, runs at batch 40
      max_batch 48: 48 x 640 x 640 x 32 x 4 = 2.52e9 >= 2^31           -> must not fuse (the gate once counted 2 bytes per element,
                    1.26e9, recorded the fusion and every forward at 41 frames or more failed with a HIP error), runs at batch 48
    Two distinct frames tiled over the batch: frames 0-1 against torch, every copy bit-identical (the last frames sit at the highest
    offsets).  About 10 GB of device memory and 3 GB of host memory."""
    H = W = 640
    ws = M.SynthWeights(0, gain=1.0)
    g = M.Graph("c2flim", 3, H, W, ws)
    x, c3 = g.input()
    a = g.conv(x, 32, 1, 1, "expand", act=M.ACT_SILU, true_cin=c3)
    y = M._c2f(g, a, 32, 1, True, "blk")
    z = g.conv(y, 8, 1, 1, "tap", act=M.ACT_NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    path = _save(g, tmp_path, "c2flim")
    assert (max_batch * H * W * 32 * 4 < 2 ** 31) == fused
    e = CE.HipEngine(path, "fp16x3", max_batch)
    names = [e.layer_kernel(e.layer_index(n), max_batch) for n in ("blk.cv1.conv", "blk.m.0.cv1.conv", "blk.m.0.cv2.conv", "blk.cv2.conv")]
    print("C2f at max_batch %d: %s" % (max_batch, names))
    if fused:
        assert names[0] == "conv_c2f16_x3_kernel" and all("fused into the C2f launch" in k for k in names[1:]), names
    else:
        assert all("c2f" not in k and "fused" not in k and "x3" in k for k in names), names
    x2 = np.random.default_rng(1).uniform(0, 1, (2, 3, H, W)).astype(np.float32)
    e.engine_inference(np.ascontiguousarray(np.concatenate([x2] * (max_batch // 2), 0)))
    got = e.fetch_activation("blk.cv2.conv", max_batch)
    e.close(); os.remove(path)
    for k in range(2, max_batch):
        assert np.array_equal(got[k], got[k % 2]), k
    Wt = {k_: torch.from_numpy(v) for k_, v in ws.store.items()}
    cv = lambda t, nm, k: F.silu(F.conv2d(t, Wt[nm + ".weight"], Wt[nm + ".bias"], padding=k // 2))
    with torch.no_grad():
        t = cv(torch.from_numpy(x2), "expand", 1)
        ys = list(cv(t, "blk.cv1.conv", 1).chunk(2, 1))
        ys.append(ys[-1] + cv(cv(ys[-1], "blk.m.0.cv1.conv", 3), "blk.m.0.cv2.conv", 3))
        want = cv(torch.cat(ys, 1), "blk.cv2.conv", 1).numpy()
    rel = rel_l2(got[:2], want)
    print("C2f at max_batch %d: rel %.2e" % (max_batch, rel))
    assert rel < 3 * X3_REL, rel


def _run_last_frame(H, W, cin, cout, s, batch, info):
    """TC.run_case's graph (input -> 1x1 expand + SiLU -> the tested 3x3 conv + SiLU -> fp32 tap) with the torch reference computed on the
    LAST frame only (its rows sit at the highest offsets): -> (rel-L2, max|diff|) of that frame; info["kernel"]: the tested layer's label."""
    ws = M.SynthWeights(0, gain=1.0)
    g = M.Graph("lastframe", 3, H, W, ws)
    x, c3 = g.input()
    a = g.conv(x, cin, 1, 1, "expand", act=M.ACT_SILU, true_cin=c3)
    y = g.conv(a, cout, 3, s, "test", act=M.ACT_SILU)
    z = g.conv(y, 8, 1, 1, "tap", act=M.ACT_NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    with tempfile.TemporaryDirectory() as d:
        path = _save(g, d, "lastframe")
        e = CE.HipEngine(path, "fp16x3", batch)
        info["kernel"] = e.layer_kernel(e.layer_index("test"), batch)
        xin = np.random.default_rng(0).uniform(0, 1, (batch, 3, H, W)).astype(np.float32)
        e.engine_inference(xin)
        got = e.fetch_activation("test", batch)[-1].copy()
        e.close()
    Wt = {k_: torch.from_numpy(v) for k_, v in ws.store.items()}
    with torch.no_grad():
        t = F.silu(F.conv2d(torch.from_numpy(xin[-1:]), Wt["expand.weight"], Wt["expand.bias"]))
        want = F.silu(F.conv2d(t, Wt["test.weight"], Wt["test.bias"], stride=s, padding=1)).numpy()[0]
    return rel_l2(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("batch", [38, 39])
def test_h8x3_at_its_offset_limit(batch):
    """conv_h8x3 addresses tensors with 32-bit byte offsets below X8_OOB = 0xF0000000 = 4,026,531,840 (4 bytes per element).  A 3x3
    64 -> 64 layer at 640 x 640 is 640 x 640 x 64 x 4 = 104,857,600 B per frame for its input and for its output:
      38 frames: 3,984,588,800 B < X8_OOB -> conv_h8x3;   39 frames: 4,089,446,400 B >= X8_OOB -> conv_x3_igemm (64-bit addressing)
    The last frame, at the highest offsets, f32-class against torch on both sides.  About 9 GB of device memory, 5 GB of host memory."""
    assert (batch * 640 * 640 * 64 * 4 < 0xF0000000) == (batch == 38)
    info = {}
    rel, mx = _run_last_frame(640, 640, 64, 64, 1, batch, info)
    print("h8x3 offset limit at %d frames: last frame rel %.2e max %.2e  %s" % (batch, rel, mx, info["kernel"]))
    assert ("conv_h8x3_kernel" if batch == 38 else "conv_x3_igemm_kernel") in info["kernel"], info
    assert rel < X3_REL and mx < 1e-4, (batch, rel, mx)


@pytest.mark.parametrize("batch", [35, 36])
def test_s2d_x3_at_its_offset_limit(batch):
    """conv_s2d_x3 takes tensors below 0x70000000 = 1,879,048,192 B (s2d_x3_fits), else the layer runs on the register-staged
    conv_s2p_x3 (per-image offsets).  A 3x3 stride-2 32 -> 64 layer on a 640 x 640 map reads 640 x 640 x 32 x 4 = 52,428,800 B per frame:
      35 frames: 1,835,008,000 B < 0x70000000 -> conv_s2d_x3;   36 frames: 1,887,436,800 B >= 0x70000000 -> conv_s2p_x3
    (both far above the 96-item floor).  The last frame f32-class against torch on both sides."""
    assert (batch * 640 * 640 * 32 * 4 < 0x70000000) == (batch == 35)
    info = {}
    rel, mx = _run_last_frame(640, 640, 32, 64, 2, batch, info)
    print("s2d x3 offset limit at %d frames: last frame rel %.2e max %.2e  %s" % (batch, rel, mx, info["kernel"]))
    assert ("conv_s2d_x3_kernel" if batch == 35 else "conv_s2p_x3_kernel") in info["kernel"], info
    assert rel < X3_REL and mx < 1e-4, (batch, rel, mx)


# ------------------------------------------------------------------------------------------------------------- default-precision fallback

def _small_graph(d, tag, mid_c, f32_out=True):
    """input -> 3x3 conv "mid" (mid_c channels, 16-bit buffer) -> 1x1 "tap" (8 channels) -> output.  mid_c = 12: the 12-channel tensor is a
    side branch that nothing reads and "tap" reads the input (every conv kernel, fp32 ones included, needs a multiple of 8 input channels)."""
    ws = M.SynthWeights(4, gain=1.0)
    g = M.Graph(tag, 3, 24, 40, ws)
    x, c3 = g.input()
    a = g.conv(x, mid_c, 3, 1, "mid", act=M.ACT_SILU, true_cin=c3)
    z = g.conv(x, 8, 1, 1, "tap", act=M.ACT_NONE, f32_out=f32_out, true_cin=c3) if mid_c % 8 else g.conv(a, 8, 1, 1, "tap", act=M.ACT_NONE, f32_out=f32_out)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    return _save(g, d, tag), ws


def test_default_precision_falls_back_to_fp32_only_for_the_split_layout(tmp_path):
    """A graph with a 12-channel 16-bit tensor cannot be held in 8-channel (hi, lo) groups: OnnxEngine(path) with no precision= runs it in
    fp32 (the other exact mode) and meets the fp32 bounds against torch."""
    path, ws = _small_graph(tmp_path, "fallback12", 12)
    with pytest.raises(Exception, match="needs multiples of 8"):
        CE.HipEngine(path, precision="fp16x3", max_batch=2)
    e = CE.OnnxEngine(path, max_batch=2)
    assert e.precision == "fp32"
    xin = np.random.default_rng(5).uniform(0, 1, (2, 3, 24, 40)).astype(np.float32)
    e.engine_inference(xin)
    got = [e.fetch_activation(n, 2) for n in ("mid", "tap")]
    e.close(); os.remove(path)
    Wt = {k_: torch.from_numpy(v).double() for k_, v in ws.store.items()}
    with torch.no_grad():
        t = torch.from_numpy(xin).double()
        want = [F.silu(F.conv2d(t, Wt["mid.weight"], Wt["mid.bias"], padding=1)).numpy(), F.conv2d(t, Wt["tap.weight"], Wt["tap.bias"]).numpy()]
    for nm, o, w in zip(("mid", "tap"), got, want):
        err, rel = float(np.abs(o - w).max()), rel_l2(o, w)
        print("12-channel graph, default precision -> fp32, %s: max|diff| %.2e rel %.2e" % (nm, err, rel))
        assert o.shape == w.shape and err <= 1e-3 * max(1.0, float(np.abs(w).max())) and rel <= 1e-5


def test_default_precision_does_not_retry_other_create_errors(tmp_path, monkeypatch):
    """HipEngine with no precision= creates the engine in fp16x3 and retries in fp32 ONLY when the split layout cannot hold the graph
    ("needs multiples of 8").  Every call of adas_engine_create is recorded: a graph that fails for another reason (its output is a
    16-bit buffer) raises after exactly one create, in fp16x3, and the 12-channel graph is created twice, fp16x3 then fp32."""
    L = CE.L
    lib = L.lib()
    real = lib.adas_engine_create
    calls = []

    def spy(path, prec, max_batch, handle):
        calls.append(int(prec))
        return real(path, prec, max_batch, handle)

    monkeypatch.setattr(lib, "adas_engine_create", spy)
    bad, _ = _small_graph(tmp_path, "badout", 16, f32_out=False)
    with pytest.raises(Exception, match="is not an fp32 buffer"):
        CE.OnnxEngine(bad, max_batch=1)
    assert calls == [L.PRECISIONS["fp16x3"]], calls
    calls.clear()
    ok, _ = _small_graph(tmp_path, "fallback12", 12)
    e = CE.OnnxEngine(ok, max_batch=1)
    assert e.precision == "fp32" and calls == [L.PRECISIONS["fp16x3"], L.PRECISIONS["fp32"]], (e.precision, calls)
    e.close()
