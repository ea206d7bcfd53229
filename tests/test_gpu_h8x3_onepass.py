"""GPU: the one-pass body of conv_h8x3_kernel (csrc/conv_halo8_x3.hip: every 32-channel chunk streamed once, hi and lo planes together),
one layer at a time, element by element against float64 -- the cases, the run and the criterion of tests/test_gpu_conv_exact.py, at the
smallest shapes that reach each of the body's paths.  Both bodies carry the label conv_h8x3_kernel<ACT>, so every case also asserts what
adas_debug_h8x3_onepass answers for its layer and batch: a case that lands on the other body fails.

  1p-1chunk   16x32  32 -> 64                 one chunk: the prologue's window is the item's last
  1p-layer1   16x32  64 -> 64  ReLU, res RB   two chunks: window buffers and ring halves swap once per item (odd chunk parity between items)
  1p-ragged   13x37  80 -> 80  SiLU, res RA   slice of wider buffers between guards: padded Cin chunk (3 chunks), trimmed wave group, ragged
                                              strips, out-of-image lanes
  1p-blocks   16x32  64 -> 256 ReLU           batch 61: two 64-channel blocks per unit, the weights switch between two items of one window
  2p-wide     40x40  64 -> 64                 batch 16: windows of more than 384 pixels (420: four window pieces per wave): the predicate
                                              refuses, the two-pass body serves it
  2p-wide5    17x91  64 -> 64                 batch 13: windows of 558 pixels, five window pieces per wave.  The smallest map and batch at
                                              which the fifth piece (window pixels 512 and up) holds pixels that outputs read (up to 523, tile
                                              1); smaller maps with such plans (4x63 at 89 frames) fill it with out-of-image lanes only
  1p-2rounds  16x32  64 -> 64                 batch 256: 512 items on 256 workgroups, every one decodes and prefetches a second tile"""
import ctypes as C_
import importlib

import pytest

from conftest import load_pkg
from test_gpu_conv_exact import LEAKY, NONE, PX3, RA, RB, RELU, RN, SILU, C, check_case

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")

MIN1, RAG1, WIDE, WIDE5 = (16, 32), (13, 37), (40, 40), (17, 91)
LABEL = "conv_h8x3_kernel<{A}>"
#        case                                                                                         one-pass body?
CASES = [(C("1p-1chunk", LABEL, MIN1, 32, 64, act=LEAKY, res=RN, batch=45, precs=PX3), True),
         (C("1p-layer1", LABEL, MIN1, 64, 64, act=RELU, res=RB, batch=45, precs=PX3), True),
         (C("1p-ragged", LABEL, RAG1, 80, 80, act=SILU, res=RA, batch=22, precs=PX3, sl=True), True),
         (C("1p-blocks", LABEL, MIN1, 64, 256, act=RELU, res=RN, batch=61, precs=PX3), True),
         (C("2p-wide", LABEL, WIDE, 64, 64, act=NONE, res=RN, batch=16, precs=PX3), False),
         (C("2p-wide5", LABEL, WIDE5, 64, 64, act=LEAKY, res=RA, batch=13, precs=PX3), False),
         (C("1p-2rounds", LABEL, MIN1, 64, 64, act=SILU, res=RN, batch=256, precs=PX3), True)]


def describe(c):
    """The layer description of a case's conv as tests/test_gpu_conv_exact.py builds it: whole buffers, or (sl) channels [8, 8 + cin) of a
    buffer of cin + 16 read and [16, 16 + cout) of one of cout + 32 written; a residual of the conv's own shape is its input."""
    h, w = c["hw"]
    cin, cout = c["cin"], c["cout"]
    x = L.MlView(0x100000, cin + 16, 8, cin, h, w) if c["sl"] else L.MlView(0x100000, cin, 0, cin, h, w)
    y = L.MlView(0x200000, cout + 32, 16, cout, h, w) if c["sl"] else L.MlView(0x200000, cout, 0, cout, h, w)
    r = L.MlView()
    if c["res"] != RN:
        r = x if cin == cout else L.MlView(0x300000, cout, 0, cout, h, w)
    return L.MlLayerDesc(1, 1, c["act"], c["res"], 0, 0, x, y, r, L.MlView())


@pytest.mark.parametrize("c,onepass", CASES, ids=[c["id"] for c, _ in CASES])
def test_h8x3_body_per_element(tmp_path, c, onepass):
    assert L.lib().adas_debug_h8x3_onepass(C_.byref(describe(c)), c["batch"]) == int(onepass)
    check_case(tmp_path, c, "fp16x3")       # (asserts the label the engine gives the layer)
