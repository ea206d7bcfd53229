"""CPU: EfficientDet-D1 / D2 / D3 (models.efficientdet under compound scaling) and the two-pass tail's logic.

  * the builders: stage tables, outputs, anchor rows, multiply-adds against the paper, and the op list through the torch interpreter
    (tests/graph_interp.py) against the independent oracle tests/effdet_oracle.py;
  * D0 untouched: the container's bytes hash to what they hashed to before the builder took a scale;
  * tests/effdet_oracle.py on D0's arguments against the pinned oracle/nets.efficientdet_forward;
  * the class-max + finish passes of csrc/post_core.h (host build, tests/hostemu/emu_effdet_scan.cpp) against oracle/effdet_tail.tail,
    bit for bit, over chunk sizes, staging tiles, threads per row and alignments.
"""
import hashlib
import importlib

import numpy as np
import pytest
import torch

import effdet_oracle as EO
import emu_effdet_scan_api as ES
import graph_interp
import netutil
from conftest import load_pkg
from oracle import nets, effdet_tail
from test_hostemu_logic import _effdet_heads

load_pkg()
M = importlib.import_module("adas_amd.models")

D0_SHA256 = "10e2e6a726692962e8bce27537a9a8c07f64a828972d684dfd9e09c7dd17ad26"      # sha256(M.build("efficientdet-d0").tobytes()) before D1-D3
STAGES = {1: (32, [(16, 2), (24, 3), (40, 3), (80, 4), (112, 4), (192, 5), (320, 2)]),
          2: (32, [(16, 2), (24, 3), (48, 3), (88, 4), (120, 4), (208, 5), (352, 2)]),
          3: (40, [(24, 2), (32, 3), (48, 3), (96, 5), (136, 5), (232, 6), (384, 2)])}
ROWS = {1: 76725, 2: 110484, 3: 150381}
PAPER_MACS = {1: 6.1e9, 2: 11e9, 3: 25e9}          # arXiv:1911.09070 table 2 ("FLOPs" there are multiply-adds)
SCALE_ROW = {1: (640, 88, 4, 3), 2: (768, 112, 5, 3), 3: (896, 160, 6, 4)}


def _build(name, **kw):
    ws = M.SynthWeights(0, gain=M.synth_gain(name))
    g = M.build(name, wsrc=ws, **kw)
    return g, dict(ws.store)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_efficientdet_scaled_builder(n):
    """Stage table, ten outputs, anchor rows, multiply-adds within 2 % of the paper's (this parameterisation: 6.040 / 10.895 / 24.691 G)."""
    name = "efficientdet-d%d" % n
    cfg = M.EFFDET_SCALES[n]
    stem, want = STAGES[n]
    assert M.round_filters(32, cfg["width"]) == stem
    assert [(c, r) for _, _, _, c, r in M.effnet_stages(cfg["width"], cfg["depth"])] == want
    assert (cfg["imgsz"], cfg["fpn_c"], cfg["fpn_cells"], cfg["head_layers"]) == SCALE_ROW[n]
    assert M.synth_gain(name) == cfg["gain"]
    g, W = _build(name)
    assert g.name == name and (g.in_h, g.in_w) == (cfg["imgsz"],) * 2
    assert W["stem.weight"].shape[0] == stem
    ends = np.cumsum([r for _, r in want])
    for (c, r), e in zip(want, ends):
        assert W["blocks.%d.project.weight" % (e - 1)].shape[0] == c and W["blocks.%d.project.weight" % (e - r)].shape[0] == c
    assert "blocks.%d.project.weight" % ends[-1] not in W
    assert "bifpn.%d.conv3_up.pw.weight" % (cfg["fpn_cells"] - 1) in W and "bifpn.%d.conv3_up.pw.weight" % cfg["fpn_cells"] not in W
    assert W["bifpn.0.p3_down.weight"].shape[0] == cfg["fpn_c"]
    assert "regressor.conv_list.%d.dw.weight" % (cfg["head_layers"] - 1) in W and "regressor.conv_list.%d.dw.weight" % cfg["head_layers"] not in W
    assert len(g.outs) == 10
    names = [o[3] for o in g.outs]
    assert names == [s + ".l%d" % l for l in range(5) for s in ("regression", "classification")], names
    assert sum(int(o[2][1]) for o in g.outs[0::2]) == ROWS[n] == sum(int(o[2][1]) for o in g.outs[1::2])
    macs = g.flops / 2
    print("%s: %.3f G multiply-adds, paper %.1f G" % (name, macs / 1e9, PAPER_MACS[n] / 1e9))
    assert abs(macs - PAPER_MACS[n]) <= 0.02 * PAPER_MACS[n], macs


@pytest.mark.parametrize("n", [1, 2, 3])
def test_efficientdet_scaled_graph_equals_oracle(n):
    """The op list of efficientdet-d<n> at 128 x 256 through the interpreter against tests/effdet_oracle.py (stage table, BiFPN width / cells
    and head depth handed to it from ITS OWN table): the ten raw head tensors, atol 2e-5 as for D0."""
    name = "efficientdet-d%d" % n
    g, W = _build(name, imgsz=(128, 256))
    x = (netutil.coco_like_frames(2, 128, 256, seed=3) - 0.45) / 0.225
    outs = graph_interp.run(g, x)
    c = EO.config(n)
    reg, cls = EO.forward(x, W, c["stages"], c["fpn_c"], c["fpn_cells"], c["head_layers"])
    got_reg = np.concatenate([o.reshape(2, -1, 4) for o in outs[0::2]], 1)
    got_cls = np.concatenate([o.reshape(2, -1, 90) for o in outs[1::2]], 1)
    n_anchors = 9 * sum((128 >> l) * (256 >> l) for l in range(3, 8))
    assert got_reg.shape == tuple(reg.shape) == (2, n_anchors, 4) and got_cls.shape == tuple(cls.shape) == (2, n_anchors, 90)
    print("%s: max |reg| %.3g, max |cls| %.3g, max deviation reg %.2e cls %.2e" % (name, float(reg.abs().max()), float(cls.abs().max()),
          float(np.abs(got_reg - reg.numpy()).max()), float(np.abs(got_cls - cls.numpy()).max())))
    np.testing.assert_allclose(got_reg, reg.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(got_cls, cls.numpy(), rtol=0, atol=2e-5)


def test_efficientdet_d0_container_is_unchanged():
    g = M.build("efficientdet-d0")
    assert g.name == "efficientdet-d0" and hashlib.sha256(g.tobytes()).hexdigest() == D0_SHA256


def test_effdet_oracle_equals_pinned_d0_oracle():
    """tests/effdet_oracle.py on D0's arguments against oracle/nets.efficientdet_forward on the same weights and frames.  Both run the same
    torch operators on the same operands in the same order, so the bound is fp32 round-off: one part in 1e6 of the tensor's range (8 ulp)."""
    g, W = _build("efficientdet-d0", imgsz=(128, 256))
    x = torch.from_numpy((netutil.coco_like_frames(2, 128, 256, seed=3) - 0.45) / 0.225)
    c = EO.config(0)
    assert c["stages"] == nets.EFFNET_B0 and (c["stem"], c["imgsz"], c["fpn_c"], c["fpn_cells"], c["head_layers"]) == (32, 512, 64, 3, 3)
    assert EO.tap_blocks(c["stages"]) == [4, 10, 15]
    t_new, t_old = {}, {}
    reg, cls = EO.forward(x, W, c["stages"], c["fpn_c"], c["fpn_cells"], c["head_layers"], taps=t_new)
    with torch.no_grad():
        reg0, cls0 = nets.efficientdet_forward(x, W, taps=t_old)
    for a, b, tag in [(reg.numpy(), reg0.numpy(), "reg"), (cls.numpy(), cls0.numpy(), "cls")] + [(t_new[k], t_old[k], k) for k in ("c3", "c4", "c5")]:
        err = float(np.abs(a - b).max())
        print("effdet oracle vs pinned D0 oracle, %s: max deviation %.2e of %.3g" % (tag, err, float(np.abs(b).max())))
        assert a.shape == b.shape and err <= 1e-6 * max(1.0, float(np.abs(b).max())), tag


# (chunk, rows staged per trip, threads per row, floats off a 16-byte boundary).  256 / 64 / 4 is what the device launches; 100 divides
# no level of any size below; 1000 exceeds the smallest level of every size (135 .. 441 anchors) and 7 is below one cell's nine anchors;
# 17 x 5: a tile that divides no chunk, five segments of 18 classes; 50 threads per row: segments of two classes, the last five empty
SCAN_CASES = [(256, 64, 4, 0), (100, 64, 4, 1), (1000, 17, 5, 3), (7, 3, 1, 2), (64, 8, 50, 2)]


@pytest.mark.parametrize("chunk,tile,parts,misalign", SCAN_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("seed,in_hw", [(0, (640, 640)), (1, (768, 768)), (2, (896, 896)), (3, (384, 640)), (4, (128, 128))], ids=lambda v: str(v))
def test_effdet_tail_two_pass(seed, in_hw, chunk, tile, parts, misalign):
    """Class-max pass over every chunk, then the finish pass (host build) against the numpy restatement: candidate count, boxes, class
    ids and confidences identical.  (128, 128): the smallest level is one cell, nine anchors."""
    reg, cls = _effdet_heads(seed, in_hw)
    want = effdet_tail.tail(reg, cls, in_hw, 0.05, 0.5, 100)
    got = ES.effdet_tail(reg, cls, in_hw, 0.05, 0.5, 100, cap=3072, chunk=chunk, tile=tile, parts=parts, misalign=misalign)
    rows = [9 * (in_hw[0] >> l) * (in_hw[1] >> l) for l in range(3, 8)]
    assert len(got["chunk_counts"]) == sum(-(-r // chunk) for r in rows) and int(got["chunk_counts"].sum()) == want["n_candidates"]
    assert got["n_candidates"] == want["n_candidates"] and 100 <= want["n_candidates"] <= 3072 and len(want["conf"]) >= 5
    np.testing.assert_array_equal(got["class_id"], want["class_id"])
    np.testing.assert_array_equal(got["conf"], want["conf"])
    np.testing.assert_array_equal(got["boxes"], want["boxes"])


def test_effdet_tail_two_pass_ties_take_the_first_class():
    """Equal logits across the segments of a row: the first class wins, as in the sequential scan."""
    reg, cls = _effdet_heads(7, (128, 128))
    cls[5::11, :] = np.float32(1.5)            # whole rows tied
    cls[3::17, 40] = cls[3::17, 80] = 2.25     # a tie between two segments (threads per row 4: classes 23 .. 45 and 69 .. 89)
    want = effdet_tail.tail(reg, cls, (128, 128), 0.05, 0.5, 2000)
    assert (want["class_id"] == 0).any() and (want["class_id"] == 40).any()      # both kinds of tie reach the output
    for chunk, tile, parts, misalign in SCAN_CASES:
        got = ES.effdet_tail(reg, cls, (128, 128), 0.05, 0.5, 2000, cap=3072, chunk=chunk, tile=tile, parts=parts, misalign=misalign)
        assert got["n_candidates"] == want["n_candidates"]
        np.testing.assert_array_equal(got["class_id"], want["class_id"])
        np.testing.assert_array_equal(got["conf"], want["conf"])
        np.testing.assert_array_equal(got["boxes"], want["boxes"])


@pytest.mark.parametrize("chunk,tile,parts,misalign", SCAN_CASES, ids=lambda v: str(v))
def test_effdet_tail_two_pass_overflow_is_reported(chunk, tile, parts, misalign):
    """More anchors over the score threshold than max_candidates: the count is reported, nothing is kept -- as the single-workgroup tail does."""
    import emu_api
    reg, cls = _effdet_heads(5, (128, 128), bias=0.0)
    old = emu_api.effdet_tail(reg, cls, (128, 128), 0.05, 0.5, 100, cap=64)
    got = ES.effdet_tail(reg, cls, (128, 128), 0.05, 0.5, 100, cap=64, chunk=chunk, tile=tile, parts=parts, misalign=misalign)
    assert got["n_candidates"] == old["n_candidates"] > 64 and len(got["conf"]) == 0
