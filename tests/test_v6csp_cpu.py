"""CPU: YOLOv6 v3.0 m / l (CSPBepBackbone, CSPRepBiFPANNeck, EffiDeHead with DFL).  The builder's sizes against upstream's published
deploy-model sizes, the builder's op list (tests/graph_interp.py) against the module-by-module oracle (tests/v6csp_oracle.py), the
BottleRep alphas' wiring, n / s containers unchanged, and the ONNX import of files written in the v3.0 exporter's vocabulary (anonymous
initializers, Mul + Add shortcuts, the Reshape / Transpose / Softmax / proj Conv DFL tail)."""
import copy, hashlib, importlib

import numpy as np
import pytest

import graph_interp as GI
import netutil
import onnx_writer as OW
import v6csp_oracle as O
from conftest import load_pkg

load_pkg()
M = importlib.import_module("adas_amd.models")
OI = importlib.import_module("adas_amd.onnx_import")

# sha256 of M.build(name).tobytes() recorded at the commit before YOLOv6 m / l were added
V6_NS_SHA256 = {"yolov6n": "bb1efd0b1019a18caa0c965906625526bcd063f07d43b1159c5fc7979a81a6a2",
                "yolov6s": "ad9b8087774015683fd563275e4eb9eefbc77c838b943fcd84466e4a6889ab9a"}
TAPS = (("sppf", "backbone.ERBlock_5.2.cv2.block.conv"), ("p3", "neck.Rep_p3.cv3.block.conv"), ("p4", "neck.Rep_n3.cv3.block.conv"),
        ("p5", "neck.Rep_n4.cv3.block.conv"))


def _synth(name, seed=0, **kw):
    ws = M.SynthWeights(seed, gain=M.synth_gain(name))
    g = M.build(name, wsrc=ws, **kw)
    return dict(ws.store), g


def _interp(g, x):
    """graph_interp on the op list without the DFL Detect op (the interpreter knows the 4-distance decode only) -> per-op taps."""
    g2 = copy.copy(g)
    g2.ops = [o for o in g.ops if o["type"] != M.OP_DETECT_V6]
    taps = {}
    GI.run(g2, x, taps)
    return taps


@pytest.mark.parametrize("name,params,gflops", [("yolov6m", 34.9, 85.8), ("yolov6l", 59.6, 150.7)])
def test_sizes_match_upstream(name, params, gflops):
    g = M.build(name)
    print(name, g.n_params / 1e6, g.flops / 1e9, g.n_convs)
    assert abs(g.n_params / 1e6 - params) <= 0.005 * params
    assert abs(g.flops / 1e9 - gflops) <= 0.015 * gflops
    assert g.meta["kind"] == "yolov6" and g.outs[0][2] == [1, 8400, 85]
    assert g.n_convs == OI.V6_CSP_CONVS[name[-1]]
    det = [o for o in g.ops if o["type"] == M.OP_DETECT_V6]
    assert len(det) == 1 and det[0]["params"][5] == 16 and all(v.c == 68 for v in det[0]["ins"][0::2])
    names = {o["name"] for o in g.ops}
    for i in range(3):
        assert {f"detect.stems.{i}.conv", f"detect.cls_convs.{i}.conv", f"detect.cls_preds.{i}", f"detect.reg_convs.{i}.conv",
                f"detect.reg_preds.{i}"} <= names
    bad = [(h, w, c) for h, w, c, fl in g.bufs if not fl & M.BUF_F32 and c % 8]
    assert not bad, bad                       # every 16-bit buffer a multiple of 8 channels: the split-precision convs take all of them


@pytest.mark.parametrize("scale", ["m", "l"])
def test_builder_matches_oracle(scale):
    name = "yolov6" + scale
    W, g = _synth(name, imgsz=(96, 160))
    x = netutil.coco_like_frames(2, 96, 160, seed=3)
    otaps = {}
    want = O.forward(x, W, scale, taps=otaps)
    assert want.shape == (2, 12 * 20 + 6 * 10 + 3 * 5, 85)
    taps = _interp(g, x)
    for key, lname in TAPS:
        a, r = taps[lname], otaps[key].numpy()
        err = float(np.abs(a - r).max())
        print(name, key, "max|diff| %.2e  max|ref| %.2f" % (err, np.abs(r).max()))
        assert a.shape == r.shape and err <= 1e-5 * max(1.0, float(np.abs(r).max())), key
    regs = [taps[f"detect.reg_preds.{i}"] for i in range(3)]
    clss = [taps[f"detect.cls_preds.{i}"] for i in range(3)]
    assert all(r.shape[1] == 68 for r in regs)
    got = O.decode_np64(regs, clss, g.meta["strides"])
    eb = float((np.abs(got[..., :4] - want[..., :4]) / (1e-3 + 1e-5 * np.abs(want[..., :4]))).max())
    ep = float(np.abs(got[..., 4:] - want[..., 4:]).max())
    print(name, "head: box %.3f of its bound, prob max|diff| %.2e" % (eb, ep))
    assert eb <= 1.0 and ep <= 1e-5


@pytest.mark.parametrize("scale", ["m", "l"])
def test_every_alpha_is_wired(scale):
    """Each BottleRep alpha (drawn in [0.6, 0.9]) set to 1 on its own changes the network's output."""
    name = "yolov6" + scale
    W, g = _synth(name, imgsz=(64, 64))
    alphas = [k for k in W if k.endswith(".alpha")]
    assert len(alphas) == {"m": 24, "l": 45}[scale]
    assert all(0.6 <= float(W[k][0]) <= 0.9 for k in alphas)
    x = netutil.coco_like_frames(1, 64, 64, seed=4)
    base = _interp(g, x)
    outs = [f"detect.{b}_preds.{i}" for b in ("reg", "cls") for i in range(3)]
    for k in alphas:
        W2 = dict(W)
        W2[k] = np.ones(1, np.float32)
        t = _interp(M.build(name, wsrc=M.DictWeights(W2), imgsz=(64, 64)), x)
        assert max(float(np.abs(t[o] - base[o]).max()) for o in outs) > 1e-6, k


@pytest.mark.parametrize("name", ["yolov6n", "yolov6s"])
def test_v6_ns_containers_unchanged(name):
    assert hashlib.sha256(M.build(name).tobytes()).hexdigest() == V6_NS_SHA256[name]


# ------------------------------------------------------------------------------------- ONNX
def _v6csp_onnx(W, path, hw=(640, 640), nc=80, proj=None, alpha_names=False):
    """A v3.0 deploy export in the exporter's vocabulary: the parameterised layers in forward order under anonymous names, each BottleRep
    shortcut a Mul by its alpha + Add, each level's reg_preds followed by the DFL tail Reshape / Transpose / Softmax / proj Conv,
    the class branch by a Sigmoid."""
    H, Wd = hw
    proj = np.arange(17, dtype=np.float32) if proj is None else np.asarray(proj, np.float32)
    inits, nodes = [OW.tensor("detect.proj_conv.weight", proj.reshape(1, 17, 1, 1))], []
    cur, k, lvl = "images", 0, 0

    def t():
        nonlocal k
        k += 1
        return "t%d" % k
    for key in W:
        if key.endswith(".alpha"):
            an = key if alpha_names else "onnx::Mul_%d" % (5000 + k)
            inits.append(OW.tensor(an, W[key]))
            y, z = t(), t()
            nodes.append(OW.node("Mul", [an, "x%d" % k], [y], "Mul_%d" % k))
            nodes.append(OW.node("Add", [cur, y], [z], "Add_%d" % k))
            cur = z
            continue
        if not key.endswith(".weight"):
            continue
        base = key[:-7]
        w, b = W[key], W[base + ".bias"]
        wn, bn = "onnx::Conv_%d" % (900 + 2 * k), "onnx::Conv_%d" % (901 + 2 * k)
        inits += [OW.tensor(wn, w), OW.tensor(bn, b)]
        op = "ConvTranspose" if "upsample_transpose" in base else "Conv"
        y = t()
        nodes.append(OW.node(op, [cur, wn, bn], [y], "%s_%d" % (op, k), [OW.attr_ints("kernel_shape", list(w.shape[2:]))]))
        cur = y
        if base.startswith("detect.cls_preds."):
            nodes.append(OW.node("Sigmoid", [cur], [t()], "Sigmoid_%d" % k))
        if base.startswith("detect.reg_preds."):
            s = 8 << lvl
            l = (H // s) * (Wd // s)
            lvl += 1
            sn = "onnx::Reshape_%d" % (7000 + k)
            inits.append(OW.tensor(sn, np.array([-1, 4, 17, l], np.int64)))
            r, tr, sm, pc = t(), t(), t(), t()
            nodes += [OW.node("Reshape", [cur, sn], [r], "Reshape_%d" % k),
                      OW.node("Transpose", [r], [tr], "Transpose_%d" % k, [OW.attr_ints("perm", [0, 2, 1, 3])]),
                      OW.node("Softmax", [tr], [sm], "Softmax_%d" % k, [OW.attr_int("axis", 1)]),
                      OW.node("Conv", [sm, "detect.proj_conv.weight"], [pc], "Conv_proj_%d" % k, [OW.attr_ints("kernel_shape", [1, 1])])]
            cur = pc
    A = sum((H // s) * (Wd // s) for s in (8, 16, 32))
    path.write_bytes(OW.model(nodes, inits, [("images", [1, 3, H, Wd])], [("outputs", [1, A, 5 + nc])]))
    return path


@pytest.mark.parametrize("scale", ["m", "l"])
def test_onnx_round_trip(tmp_path, scale):
    name = "yolov6" + scale
    W, g = _synth(name, seed=3)
    p = _v6csp_onnx(W, tmp_path / (name + ".onnx"))
    m = OI.read_onnx(str(p))
    assert OI.detect_arch(m) == (name, dict(nc=80, imgsz=(640, 640)))
    out, g2 = OI.convert(str(p), str(tmp_path / (name + ".hipm")))
    assert g2.name == name and g2.tobytes() == M.build(name, wsrc=M.DictWeights(W)).tobytes()


def test_onnx_named_alphas_are_cross_checked(tmp_path):
    """An export that keeps upstream's alpha names: taken by position, and each named tensor must be the one at its position."""
    W, g = _synth("yolov6m", seed=5, imgsz=(96, 160))
    p = _v6csp_onnx(W, tmp_path / "named.onnx", hw=(96, 160), alpha_names=True)
    _, g2 = OI.convert(str(p), str(tmp_path / "named.hipm"))
    assert g2.tobytes() == M.build("yolov6m", wsrc=M.DictWeights(W), imgsz=(96, 160)).tobytes()
    keys = [k for k in W if k.endswith(".alpha")]
    m = OI.read_onnx(str(_v6csp_onnx(W, tmp_path / "anon.onnx", hw=(96, 160))))
    m.initializers.update({keys[3]: W[keys[4]], keys[4]: W[keys[3]]})     # named copies that disagree with the graph positions
    with pytest.raises(ValueError, match="alpha"):
        M.build("yolov6m", wsrc=OI.OnnxWeights(m, "yolov6m"), imgsz=(96, 160))


def test_onnx_wrong_proj_refused(tmp_path):
    W, g = _synth("yolov6m", seed=3, imgsz=(96, 160))
    p = _v6csp_onnx(W, tmp_path / "proj.onnx", hw=(96, 160), proj=np.arange(1, 18))
    m = OI.read_onnx(str(p))
    assert OI.detect_arch(m)[0] == "yolov6m"
    with pytest.raises(ValueError, match="proj_conv"):
        OI.OnnxWeights(m, "yolov6m")
    with pytest.raises(ValueError, match="proj_conv"):
        OI.convert(str(p), str(tmp_path / "proj.hipm"))


def test_onnx_other_v6_width_refused_by_name(tmp_path):
    W, g = _synth("yolov6m", seed=3, imgsz=(96, 160))
    W = dict(W)
    W["backbone.stem.rbr_reparam.weight"] = np.zeros((40, 3, 3, 3), np.float32)
    W["backbone.stem.rbr_reparam.bias"] = np.zeros(40, np.float32)
    m = OI.read_onnx(str(_v6csp_onnx(W, tmp_path / "v6_40.onnx", hw=(96, 160))))
    with pytest.raises(ValueError, match="yolov6n / yolov6s.*yolov6m / yolov6l"):
        OI.detect_arch(m)
