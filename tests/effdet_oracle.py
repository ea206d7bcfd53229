"""Oracle: torch-CPU fp32 forward of the scaled EfficientDets (D0 .. D3), module by module (test infrastructure; shares nothing with
models.py).

Restates the published architecture from its description: EfficientNet under compound scaling (Tan & Le, arXiv:1905.11946: table 1's
seven MBConv stages, section 3.3's width / depth coefficients, channels through round_filters -- nearest multiple of 8, never more than
10 % below -- and repeats ceil(depth * n); squeeze-and-excitation of a quarter of the block's INPUT channels; swish; identity skip when
stride 1 and in == out), the BiFPN (Tan, Pang, Le, arXiv:1911.09070 section 3: fast normalised fusion eq. 3, P6 / P7 by 3x3 stride-2
max-pooling of a 1x1 projection of C5, the first cell re-projecting C4 / C5 for its bottom-up path, nearest 2x upsampling) and the class /
box heads (section 4: depth-wise + point-wise layers shared by the five levels, BatchNorm per level -- folded into the point-wise
parameters --, a header without BatchNorm; 9 anchors per cell), symmetric k // 2 padding.

Arguments of forward(): the stage table [(expand, kernel, stride, out channels, repeats)], the stem width, the BiFPN width / cell count and
the head depth; weights by name (the names oracle/nets.efficientdet_forward reads, which pins this file to it on D0's arguments:
tests/test_effdet_scaled_cpu.py).  Rounding emulation (oracle.nets.EMULATE) passes through oracle.nets._round at every stored activation.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets
from oracle.nets import _conv, _dwconv, _t

B0_STAGES = [(1, 3, 1, 16, 1), (6, 3, 2, 24, 2), (6, 5, 2, 40, 2), (6, 3, 2, 80, 3), (6, 5, 1, 112, 3), (6, 5, 2, 192, 4), (6, 3, 1, 320, 1)]
# arXiv:1911.09070 table 1: backbone (width, depth) coefficients, input size, BiFPN width, BiFPN cells, head layers
TABLE = {0: (1.0, 1.0, 512, 64, 3, 3), 1: (1.0, 1.1, 640, 88, 4, 3), 2: (1.1, 1.2, 768, 112, 5, 3), 3: (1.2, 1.4, 896, 160, 6, 4)}


def round_filters(c, width):
    v = c * width
    r = max(8, int(v + 4) // 8 * 8)
    if r < 0.9 * v:
        r += 8
    return r


def stages(width, depth):
    return [(e, k, s, round_filters(c, width), int(math.ceil(depth * n))) for e, k, s, c, n in B0_STAGES]


def config(scale):
    """-> dict(stages, stem, imgsz, fpn_c, fpn_cells, head_layers) of EfficientDet-D<scale>."""
    w, d, imgsz, fc, cells, hl = TABLE[scale]
    return dict(stages=stages(w, d), stem=round_filters(32, w), imgsz=imgsz, fpn_c=fc, fpn_cells=cells, head_layers=hl)


def tap_blocks(stage_table):
    """Names' block indices of the last MBConv of stages 3, 5 and 7 (the C3 / C4 / C5 features)."""
    ends = np.cumsum([n for *_, n in stage_table])
    return [int(ends[i]) - 1 for i in (2, 4, 6)]


def _r(t):
    return nets._round(t)       # reads oracle.nets.EMULATE at call time


def _se(x, W, name):
    m = x.mean((2, 3), keepdim=True)
    h = F.silu(F.conv2d(m, _t(W, name + ".reduce.weight"), _t(W, name + ".reduce.bias")))
    gate = torch.sigmoid(F.conv2d(h, _t(W, name + ".expand.weight"), _t(W, name + ".expand.bias")))
    return _r(x * gate)


def _mbconv(x, W, name, e, s, cout):
    cin = x.shape[1]
    t = _conv(x, W, name + ".expand") if e != 1 else x
    t = _se(_dwconv(t, W, name + ".dw", s), W, name + ".se")
    t = _conv(t, W, name + ".project", act=None)
    return _r(t + x) if (s == 1 and cin == cout) else _r(t)


def _sep(x, W, name, act=None, dw_name=None, last=False):
    """depth-wise 3x3 without bias -> point-wise 1x1 with bias [-> swish]; the header's fp32 output (last) is not a stored 16-bit map."""
    w = _r(_t(W, (dw_name or name) + ".dw.weight"))
    t = _r(F.conv2d(x, w, None, padding=1, groups=x.shape[1]))
    y = _conv(t, W, name + ".pw", act=act)
    return y if last else _r(y)


def _fusion(W, name):
    w = np.maximum(np.asarray(W[name], np.float32), np.float32(0))
    return (w / (w.sum(dtype=np.float32) + np.float32(1e-4))).astype(np.float32)


def backbone(x, W, stage_table):
    """-> [C3, C4, C5]"""
    t = _conv(x, W, "stem", s=2)
    feats, bi = [], 0
    for si, (e, k, s, c, n) in enumerate(stage_table):
        for r in range(n):
            t = _mbconv(t, W, "blocks.%d" % bi, e, s if r == 0 else 1, c)
            bi += 1
        if si in (2, 4, 6):
            feats.append(t)
    return feats


def bifpn(feats, W, cells):
    c3, c4, c5 = feats
    up = lambda v: F.interpolate(v, scale_factor=2, mode="nearest")
    down = lambda v: F.max_pool2d(v, 3, 2, 1)
    p = None
    for cell in range(cells):
        nm = "bifpn.%d" % cell
        if cell == 0:
            p3, p4, p5 = (_r(_conv(c, W, "%s.p%d_down" % (nm, 3 + i), act=None)) for i, c in enumerate((c3, c4, c5)))
            p6 = down(_r(_conv(c5, W, nm + ".p5_to_p6", act=None)))
            p7 = down(p6)
            p4b, p5b = _r(_conv(c4, W, nm + ".p4_down_2", act=None)), _r(_conv(c5, W, nm + ".p5_down_2", act=None))
        else:
            p3, p4, p5, p6, p7 = p
            p4b, p5b = p4, p5

        def node(tag, conv, ins):
            acc = 0
            for wi, v in zip(_fusion(W, "%s.%s" % (nm, tag)), ins):
                acc = acc + float(wi) * v
            return _sep(_r(F.silu(acc)), W, "%s.%s" % (nm, conv))

        p6u = node("p6_w1", "conv6_up", [p6, up(p7)])
        p5u = node("p5_w1", "conv5_up", [p5, up(p6u)])
        p4u = node("p4_w1", "conv4_up", [p4, up(p5u)])
        p3o = node("p3_w1", "conv3_up", [p3, up(p4u)])
        p4o = node("p4_w2", "conv4_down", [p4b, p4u, down(p3o)])
        p5o = node("p5_w2", "conv5_down", [p5b, p5u, down(p4o)])
        p6o = node("p6_w2", "conv6_down", [p6, p6u, down(p5o)])
        p7o = node("p7_w2", "conv7_down", [p7, down(p6o)])
        p = (p3o, p4o, p5o, p6o, p7o)
    return p


def heads(p, W, head_layers, nc):
    """-> (regression (N, A, 4), class logits (N, A, nc)), rows (level, y, x, anchor)."""
    out = {"regressor": [], "classifier": []}
    for lv, f in enumerate(p):
        for branch, per in (("regressor", 4), ("classifier", nc)):
            t = f
            for i in range(head_layers):
                t = _sep(t, W, "%s.l%d.%d" % (branch, lv, i), act="silu", dw_name="%s.conv_list.%d" % (branch, i))
            o = _sep(t, W, "%s.l%d.header" % (branch, lv), dw_name=branch + ".header", last=True)
            out[branch].append(o.permute(0, 2, 3, 1).reshape(o.shape[0], -1, per))
    return torch.cat(out["regressor"], 1), torch.cat(out["classifier"], 1)


def forward(x, W, stage_table, fpn_c, fpn_cells, head_layers, nc=90, taps=None):
    """x (N, 3, H, W) fp32 -> (regression (N, A, 4) as (dy, dx, dh, dw), class logits (N, A, nc)) torch tensors.
    taps: filled with c3 / c4 / c5 as numpy arrays.  fpn_c is implied by the weights' shapes and only checked."""
    x = torch.as_tensor(x, dtype=torch.float32)
    with torch.no_grad():
        feats = backbone(x, W, stage_table)
        if taps is not None:
            taps.update(c3=feats[0].numpy().copy(), c4=feats[1].numpy().copy(), c5=feats[2].numpy().copy())
        p = bifpn(feats, W, fpn_cells)
        assert all(v.shape[1] == fpn_c for v in p), [v.shape for v in p]
        return heads(p, W, head_layers, nc)


def forward_scale(x, W, scale, nc=90, taps=None):
    c = config(scale)
    return forward(x, W, c["stages"], c["fpn_c"], c["fpn_cells"], c["head_layers"], nc, taps)
