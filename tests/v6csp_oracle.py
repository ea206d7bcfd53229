"""Oracle: torch-CPU fp32 forward of YOLOv6 v3.0 m / l, module by module (test infrastructure; shares nothing with models.py).

Restates meituan/YOLOv6 v3.0 in deploy form: configs/yolov6m.py / yolov6l.py (depth 0.60 / 1.0, width 0.75 / 1.0, csp_e 2/3 / 1/2,
training_mode repvgg / conv_silu, num_repeats [1, 6, 12, 18, 6] + [12, 12, 12, 12], fuse_P2, use_dfl True, reg_max 16),
yolov6/models/yolo.py build_network (make_divisible(c * width, 8), repeats max(round(n * depth), 1)), efficientrep.py CSPBepBackbone
(SimSPPF behind RepVGGBlock, SPPF behind ConvBNSiLU), reppan.py CSPRepBiFPANNeck, layers/common.py BepC3 / RepBlock(block=BottleRep) /
BottleRep / BiFusion / Transpose, effidehead.py Detect.forward (eval branch, DFL: reshape(-1, 4, 17, l).permute(0, 2, 1, 3), softmax over
the bins, proj_conv with linspace(0, 16, 17)), assigners/anchor_generator.py generate_anchors (af, offset 0.5) and utils/general.py
dist2bbox ('xywh').  Weights: a dict name -> ndarray (BatchNorm folded), the names models.yolov6_csp requests.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.nets import _conv, _round, _t, _v6_bifusion

SCALES = {"m": dict(depth=0.60, width=0.75, csp_e=float(2) / 3, mode="repvgg"),
          "l": dict(depth=1.0, width=1.0, csp_e=float(1) / 2, mode="conv_silu")}
REG_MAX = 16


def _make_divisible(x, d=8):
    return math.ceil(x / d) * d


class _Net:
    def __init__(self, W, scale):
        cfg = SCALES[scale]
        self.W, self.e = W, cfg["csp_e"]
        self.silu = cfg["mode"] == "conv_silu"
        rn = lambda n: (max(round(n * cfg["depth"]), 1) if n > 1 else n)
        self.rep = [rn(n) for n in (1, 6, 12, 18, 6, 12, 12, 12, 12)]
        self.ch = [_make_divisible(c * cfg["width"]) for c in (64, 128, 256, 512, 1024, 256, 128, 128, 256, 256, 512)]

    # layers/common.py
    def block(self, x, name, s=1):
        """RepVGGBlock (deploy: rbr_reparam 3x3 + ReLU) | ConvBNSiLU (block.conv 3x3 + SiLU)."""
        if self.silu:
            return _conv(x, self.W, name + ".block.conv", s, act="silu")
        return _conv(x, self.W, name + ".rbr_reparam", s, act="relu")

    def cbx(self, x, name, s=1):
        """BepC3's / the SPP's ConvBNReLU | ConvBNSiLU (ConvBNSiLU when the block is)."""
        return _conv(x, self.W, name + ".block.conv", s, act="silu" if self.silu else "relu")

    def cbr(self, x, name, s=1):
        return _conv(x, self.W, name + ".block.conv", s, act="relu")

    def bottlerep(self, x, name):
        out = self.block(self.block(x, name + ".conv1"), name + ".conv2")
        return _round(out + _t(self.W, name + ".alpha") * x)

    def repblock(self, x, name, n):
        x = self.bottlerep(x, name + ".conv1")
        for i in range(n // 2 - 1):
            x = self.bottlerep(x, f"{name}.block.{i}")
        return x

    def bepc3(self, x, name, n):
        return self.cbx(torch.cat((self.repblock(self.cbx(x, name + ".cv1"), name + ".m", n), self.cbx(x, name + ".cv2")), 1), name + ".cv3")

    def sppf(self, x, name):
        """SimSPPF | SPPF, kernel 5."""
        x = self.cbx(x, name + ".cv1")
        y1 = F.max_pool2d(x, 5, 1, 2)
        y2 = F.max_pool2d(y1, 5, 1, 2)
        return self.cbx(torch.cat((x, y1, y2, F.max_pool2d(y2, 5, 1, 2)), 1), name + ".cv2")

    # efficientrep.py CSPBepBackbone.forward
    def backbone(self, x):
        x = self.block(x, "backbone.stem", 2)
        outs = []
        for i in range(1, 5):
            x = self.bepc3(self.block(x, f"backbone.ERBlock_{i + 1}.0", 2), f"backbone.ERBlock_{i + 1}.1", self.rep[i])
            if i == 4:
                x = self.sppf(x, "backbone.ERBlock_5.2")
            outs.append(x)
        return outs

    # reppan.py CSPRepBiFPANNeck.forward
    def neck(self, x3, x2, x1, x0):
        W, r = self.W, self.rep
        fpn_out0 = self.cbr(x0, "neck.reduce_layer0")
        f_out0 = self.bepc3(_v6_bifusion([fpn_out0, x1, x2], W, "neck.Bifusion0"), "neck.Rep_p4", r[5])
        fpn_out1 = self.cbr(f_out0, "neck.reduce_layer1")
        pan_out2 = self.bepc3(_v6_bifusion([fpn_out1, x2, x3], W, "neck.Bifusion1"), "neck.Rep_p3", r[6])
        pan_out1 = self.bepc3(torch.cat([self.cbr(pan_out2, "neck.downsample2", 2), fpn_out1], 1), "neck.Rep_n3", r[7])
        pan_out0 = self.bepc3(torch.cat([self.cbr(pan_out1, "neck.downsample1", 2), fpn_out0], 1), "neck.Rep_n4", r[8])
        return pan_out2, pan_out1, pan_out0


def head_maps(feats, W, nc=80):
    """EffiDeHead's per-level raw predictor outputs: [(reg_preds (N, 68, h, w), cls_preds (N, nc, h, w))]."""
    out = []
    for i, f in enumerate(feats):
        st = _conv(f, W, f"detect.stems.{i}.conv")
        cls = _conv(_conv(st, W, f"detect.cls_convs.{i}.conv"), W, f"detect.cls_preds.{i}", act=None)
        reg = _conv(_conv(st, W, f"detect.reg_convs.{i}.conv"), W, f"detect.reg_preds.{i}", act=None)
        out.append((reg, cls))
    return out


def decode(maps, strides):
    """effidehead.py Detect.forward (eval, use_dfl): maps [(reg (N, 4 (R+1), h, w), cls (N, nc, h, w))] -> (N, A, 5 + nc)."""
    proj = torch.linspace(0, REG_MAX, REG_MAX + 1).view(1, REG_MAX + 1, 1, 1)
    cls_l, reg_l, pts, strd = [], [], [], []
    for (reg, cls), s in zip(maps, strides):
        b, _, h, w = cls.shape
        l = h * w
        r = reg.reshape([-1, 4, REG_MAX + 1, l]).permute(0, 2, 1, 3)
        r = F.conv2d(F.softmax(r, dim=1), proj)
        cls_l.append(torch.sigmoid(cls).reshape(b, -1, l))
        reg_l.append(r.reshape(b, 4, l))
        sy, sx = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5, indexing="ij")
        pts.append(torch.stack((sx, sy), -1).reshape(-1, 2))
        strd.append(torch.full((l, 1), float(s)))
    cls_score = torch.cat(cls_l, -1).permute(0, 2, 1)
    dist = torch.cat(reg_l, -1).permute(0, 2, 1)
    anchor_points, stride_tensor = torch.cat(pts), torch.cat(strd)
    x1y1, x2y2 = anchor_points - dist[..., :2], anchor_points + dist[..., 2:]
    boxes = torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), -1) * stride_tensor
    return torch.cat((boxes, torch.ones(boxes.shape[0], boxes.shape[1], 1), cls_score), -1)


def decode_np64(regs, clss, strides):
    """The same decode in float64 numpy: regs / clss lists of (N, 68, h, w) / (N, nc, h, w) arrays -> (N, A, 5 + nc)."""
    rows = []
    for reg, cls, s in zip(regs, clss, strides):
        reg, cls = np.asarray(reg, np.float64), np.asarray(cls, np.float64)
        n, _, h, w = cls.shape
        z = reg.reshape(n, 4, REG_MAX + 1, h * w)
        z = z - z.max(axis=2, keepdims=True)
        p = np.exp(z)
        p /= p.sum(axis=2, keepdims=True)
        d = (p * np.arange(REG_MAX + 1, dtype=np.float64).reshape(1, 1, -1, 1)).sum(axis=2)      # (n, 4, l)
        gy, gx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        ax, ay = gx.reshape(-1), gy.reshape(-1)
        x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
        box = np.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), -1) * s
        prob = 1.0 / (1.0 + np.exp(-cls.reshape(n, -1, h * w).transpose(0, 2, 1)))
        rows.append(np.concatenate((box, np.ones((n, h * w, 1)), prob), -1))
    return np.concatenate(rows, 1)


def forward(x, W, scale="m", nc=80, taps=None):
    """x: (N, 3, H, W) fp32 -> (N, A, 5 + nc) numpy: [cx, cy, w, h] in input pixels, objectness 1, class probabilities.
    taps: filled with p3 / p4 / p5 (the neck outputs) and sppf (the P5 channel merge) as torch tensors."""
    net = _Net(W, scale)
    x = torch.as_tensor(x, dtype=torch.float32)
    H_in = x.shape[2]
    with torch.no_grad():
        x3, x2, x1, x0 = net.backbone(x)
        feats = net.neck(x3, x2, x1, x0)
        if taps is not None:
            taps.update(p3=feats[0], p4=feats[1], p5=feats[2], sppf=x0)
        return decode(head_maps(feats, W, nc), [H_in // f.shape[2] for f in feats]).numpy()
