"""GPU: every 16-bit, fp32 and fp16x3 conv kernel, ONE layer at a time, element by element against float64 (tests/conv_ref.py: half an
ulp of the storage type plus K_CONV fp32 roundings of the magnitudes that enter the element, K_CONV from a float32 yardstick measured
on the CPU; nothing read off the device enters the bound).  tests/test_gpu_conv.py and test_gpu_x3.py judge the same kernels by a
whole-tensor norm behind two layers' rounding on non-negative inputs; tests/test_conv_ref_cpu.py shows what that lets through.

Pattern: a unit graph  input -> 1x1 "expand" (no activation: signed values) -> the conv under test -> 1x1 fp32 "tap"  (a conv with a
float32 output is the graph's output itself; a stem reads the input layer).  The conv's INPUT, its residual and its OUTPUT are fetched
and the reference is applied to the fetched input with the weights rounded as the engine stores them, so the comparison holds one
layer's arithmetic and one store.  Frames are uniform(-1, 1), all distinct; 3 of them unless the kernel is only dispatched at a larger batch.  Where
the float64 reference of a whole batch would take more than about a second (distinct()), as many frames as fit are distinct and repeat
with an odd period: every copy must equal its original bit for bit, and the reference is computed for the distinct ones.  The kernel label
(adas_engine_layer_kernel) is asserted: a case that lands on another kernel fails.  Slice cases read channels [8, 8 + cin) of a wider
buffer and write [16, 16 + cout) of a concat buffer between guard channels set to 7.0 in front of the conv (test_gpu_ops_exact.py).

The fused launches (conv_c2f16*, conv_pair_kernel, stem + second conv, +pool, +shortcut), whose intermediate never reaches memory, are
checked per element by tests/test_gpu_fused_exact.py: the intermediate is computed in float64 from the fetched input and rounded as the
kernel stores it (tests/fused_ref.py); that file also says where the fused Detect kernels are tested.  conv_ml_kernel and
conv_halo_group_kernel are asserted bit-identical to the per-layer launches by tests/test_gpu_ml.py and inherit this coverage.

Where the activation is a template parameter of the kernel ({A}) the cases of a label run SiLU, ReLU, leaky and none between them; fc_kernel,
conv_pw*, conv_pwg, conv_igemm and the generic fp16x3 kernels take it at run time.

label -> cases (-m: minimal, -r: ragged in every dimension the kernel admits; further epilogues and paths after them).  {A}: the activation
  conv_halo_kernel<16|32|48|64,{A},s1,bm128>   halo16-m/r  halo32-m/r  halo48-m/r  halo64-m/r;  halo-narrow (64 channels packed for 16), halo-f32
  conv_halo_kernel<16|32|48|64,{A},s1>         halo16w-m/r  halo32w-m/r  halo48w-m/r  halo64w-m/r   (256-pixel tiles: 320 workgroups and more)
  conv_halo_kernel<16|32|48|64,{A},s2>         halo16s2-m/r  halo32s2-m/r  halo48s2-m/r  halo64s2-m/r
  conv_halo_rw_kernel<1|2,{A},bn32>            rw1n-m/r  rw2n-m/r
  conv_halo_rw_kernel<1|2,{A}>                 rw1-m/r  rw2-m/r
  conv_s2p_kernel<{A}>                         s2p-m/r;  s2p-leaky, s2p-none
  conv_h8_kernel<{A}>                          h8-m/r  h8-512;  h8-leaky, h8-none
  conv_pw_kernel<1|2|3|4|5|6|8|10|12|16>       pw<KS>-m/r   (pw2-r: the ragged last step at 40 channels; pw4-m, pw8-m, pw3-r: stride 2; KS 12, 16: the
                                               output cut into ranges; float32 outputs and slices among them)
  conv_pwg_kernel<64|128>                      pwg64-m/r  pwg128-m/r;  pwg64-res
  fc_kernel                                    fc-1  fc-17  fc-17-f32  fc-wide
  conv_stem_kernel<3|6|7,n,{A}>                stem3-m/r  stem6-m/r  stem7-m/r   (a label here is the <kh> family: n follows Cout, 1 and 3 for the two 3x3 cases)
  conv_igemm_kernel<f16|bf16,same,BM,BN>       ig64x16  ig64x32  ig64x64  ig128x16  ig128x32  ig128x64  ig128x128, each -m/r;  ig-1x1-res
  conv_igemm_kernel<f16|bf16,f32,BM,BN>        the same seven tiles, -m-f32 / -r-f32
  conv_igemm_kernel<f32,f32,BM,BN>  (fp32)     ig64x16 ... ig128x64 -m/r in fp32 mode;  ig-1x1-res, ig-3x3-f32mode, ig-s2-f32mode
  conv_stem_x3_kernel<3|6|7,n,{A}>             the stem cases in fp16x3
  conv_pwx3_kernel<1|...|16>                   the pw cases in fp16x3
  fc_x3_kernel                                 the fc cases in fp16x3
  conv_h8x3_kernel<{A}>                        h8x3-m/r;  h8x3-leaky, h8x3-none
  conv_s2d_x3_kernel<{A}>                      s2d-m/r;  s2d-leaky, s2d-none
  conv_s2p_x3_kernel<{A}>                      s2px3-m/r;  s2px3-silu, s2px3-relu   (more than 32 blocks of 64 output channels: the register-staged form)
  conv_x3_ksplit_kernel                        ks-m/r;  ks-s2, ks-wide (its 32 x 64 tiles)
  conv_x3_ksplit_kernel<f32>                   ksf-m/r
  conv_x3_igemm_kernel<BM,BN>                  x3ig64x16  x3ig128x16  x3ig32x32  x3ig64x32  x3ig128x32  x3ig32x64  x3ig64x64  x3ig128x64, each -m/r
  conv_x3_igemm_kernel<BM,BN,f32>              the same eight tiles, -m-f32 / -r-f32"""
import importlib

import numpy as np
import pytest

import conv_ref as CR
import ops_ref as R
from conftest import load_pkg
from test_gpu_ops_exact import _check_guards, _guarded

pytestmark = pytest.mark.gpu
load_pkg()
CE = importlib.import_module("adas_amd.coreEngine")
M = importlib.import_module("adas_amd.models")

assert (M.ACT_NONE, M.ACT_SILU, M.ACT_RELU, M.ACT_LEAKY) == (R.ACT_NONE, R.ACT_SILU, R.ACT_RELU, R.ACT_LEAKY)
assert (M.RES_NONE, M.RES_AFTER_ACT, M.RES_BEFORE_ACT) == (CR.RES_NONE, CR.RES_AFTER_ACT, CR.RES_BEFORE_ACT)

NONE, SILU, RELU, LEAKY = R.ACT_NONE, R.ACT_SILU, R.ACT_RELU, R.ACT_LEAKY
RN, RA, RB = CR.RES_NONE, CR.RES_AFTER_ACT, CR.RES_BEFORE_ACT
ACT_TAG = {NONE: "NONE", SILU: "SILU", RELU: "RELU", LEAKY: "LEAKY"}
ELEM_TAG = {"fp16": "f16", "bf16": "bf16", "fp32": "f32"}
P16, P32, PX3 = ("fp16", "bf16"), ("fp32",), ("fp16x3",)
DISTINCT = 3                 # frames of a case that needs no batch
REF_FLOPS = 3.0e9            # float64 work the reference of one case may take (a second or two): how many frames of a batch are distinct


def C(cid, label, hw, cin, cout, k=3, s=1, act=SILU, res=RN, batch=DISTINCT, f32=False, sl=False, precs=P16, stem=False, pad=None):
    """One case: `label` is the kernel the layer must resolve to ({A}: the activation's tag, {E}: the element's)."""
    return dict(id=cid, label=label, hw=hw, cin=cin, cout=cout, k=k, s=s, act=act, res=res, batch=batch, f32=f32, sl=sl, precs=precs, stem=stem,
                pad=k // 2 if pad is None else pad)


MIN1, RAG1 = (16, 32), (13, 37)      # stride 1: 512 pixels = two 256-pixel tiles a frame; 481 pixels, no multiple of any tile or strip
MIN2, RAG2 = (16, 64), (23, 37)      # stride 2 (3x3, pad 1): outputs 8 x 32 = 256 pixels and 12 x 19 = 228 (odd inputs: the last window row / column is padding);
                                     # a smaller ragged output fills under 60 % of its tiles and leaves conv_halo (plan_halo's eff)
PWM, PWR = (12, 20), (11, 13)        # 1x1 and generic convs: 240 and 143 pixels a frame (no multiple of 16)

CASES = []
# ---- conv_halo_kernel (conv_halo.hip): 3x3, pad 1, Cin >= 16, 16-bit.  BN = halo_bn(cout): <= 16 -> 16, <= 32 -> 32, 65..96 -> 48, else 64 --
# unless plan_halo_bn narrows it: while tiles128 * ceil(cout / BN) < 256 (tiles128: the batch's 128-pixel tiles at stride 1, its 128-pixel
# tiles at stride 2) BN halves, so the natural BN of a small map needs a batch.  bm128: stride 1 and frames * tiles256 * ceil(cout / BN) < 320.
# Cin = 96 keeps the layers off conv_halo_rw (Cin <= 64) and Cout % 128 != 0 off conv_h8 / conv_s2p.  Three 32-channel K chunks.
#              id            BN  cout  batch(bm128)  batch(wide)  batch(s2)  epilogues
for bn, cout, nb, nw, n2, (e1, e2, e3, e4) in ((16, 16, 3, 160, 3, ((SILU, RN), (RELU, RB), (NONE, RN), (LEAKY, RA))),
                                           (32, 32, 64, 160, 128, ((RELU, RA), (LEAKY, RN), (SILU, RB), (NONE, RB))),
                                           (48, 80, 32, 80, 64, ((LEAKY, RB), (SILU, RA), (RELU, RN), (NONE, RA))),
                                           (64, 64, 64, 160, 128, ((NONE, RA), (SILU, RN), (LEAKY, RA), (RELU, RB)))):      # (every BN sees all four activations)
    rc = {16: 8, 32: 24, 48: 72, 64: 56}[bn]           # ragged: Cin 40 (five 8-channel groups, the last chunk a quarter full), Cout no multiple of 16 (of 8: the tap reads it)
    CASES += [C("halo%d-m" % bn, "conv_halo_kernel<%d,{A},s1,bm128>" % bn, MIN1, 96, cout, act=e1[0], res=e1[1], batch=nb),
              C("halo%d-r" % bn, "conv_halo_kernel<%d,{A},s1,bm128>" % bn, RAG1, 40, rc, act=e2[0], res=e2[1], batch=nb + 1, sl=bn in (32, 64)),
              C("halo%dw-m" % bn, "conv_halo_kernel<%d,{A},s1>" % bn, MIN1, 96, cout, act=e2[0], res=e2[1], batch=nw),
              C("halo%dw-r" % bn, "conv_halo_kernel<%d,{A},s1>" % bn, RAG1, 40, rc, act=e4[0], res=e4[1], batch=nw + 1),
              C("halo%ds2-m" % bn, "conv_halo_kernel<%d,{A},s2>" % bn, MIN2, 96, cout, s=2, act=e3[0], res=e3[1], batch=n2),
              C("halo%ds2-r" % bn, "conv_halo_kernel<%d,{A},s2>" % bn, RAG2, 40, rc, s=2, act=e1[0], res=e1[1], batch=n2 + 1, sl=bn == 48)]
CASES += [C("halo-narrow", "conv_halo_kernel<16,{A},s1,bm128>", RAG1, 96, 64, act=SILU, res=RN),          # 3 frames: 64 channels packed as four 16-wide blocks
          C("halo-f32", "conv_halo_kernel<16,{A},s1,bm128>", RAG1, 40, 12, act=NONE, f32=True)]
# ---- conv_halo_rw_kernel (conv_halo_rw.hip): 3x3 s1, 16 <= Cin <= 64, Cout > 16, BN != 48, frames * tiles * ceil(cout / BN) >= 1024 (persistent:
# every workgroup walks several tiles).  <NCH = ceil(cin / 32)>, bn32: Cout <= 32.  Ragged batches leave the workgroups uneven item lists.
CASES += [C("rw1n-m", "conv_halo_rw_kernel<1,{A},bn32>", MIN1, 32, 32, act=SILU, res=RA, batch=512),
          C("rw1n-r", "conv_halo_rw_kernel<1,{A},bn32>", RAG1, 24, 24, act=RELU, res=RN, batch=523),
          C("rw2n-m", "conv_halo_rw_kernel<2,{A},bn32>", MIN1, 64, 32, act=LEAKY, res=RB, batch=512),
          C("rw2n-r", "conv_halo_rw_kernel<2,{A},bn32>", RAG1, 40, 24, act=NONE, res=RN, batch=523, sl=True),
          C("rw1-m", "conv_halo_rw_kernel<1,{A}>", MIN1, 32, 128, act=LEAKY, res=RB, batch=256),
          C("rw1-r", "conv_halo_rw_kernel<1,{A}>", RAG1, 24, 56, act=NONE, res=RA, batch=523, sl=True),
          C("rw2-m", "conv_halo_rw_kernel<2,{A}>", MIN1, 64, 64, act=SILU, res=RA, batch=512),
          C("rw2-r", "conv_halo_rw_kernel<2,{A}>", RAG1, 40, 104, act=RELU, res=RN, batch=261)]      # (each NCH and each BN form sees the four activations)
# ---- conv_s2p_kernel (conv_halo_s2.hip): 3x3 s2, Cin >= 128, Cout % 128 == 0, no residual, frames * tiles256 * (cout / 128) >= 512
CASES += [C("s2p-m", "conv_s2p_kernel<{A}>", MIN2, 128, 256, s=2, act=RELU, batch=256),
          C("s2p-r", "conv_s2p_kernel<{A}>", RAG2, 136, 256, s=2, act=SILU, batch=257, sl=True),
          C("s2p-leaky", "conv_s2p_kernel<{A}>", MIN2, 128, 256, s=2, act=LEAKY, batch=256, sl=True),
          C("s2p-none", "conv_s2p_kernel<{A}>", MIN2, 128, 256, s=2, act=NONE, batch=256)]
# ---- conv_h8_kernel (conv_halo8.hip): 3x3 s1, Cin >= 64 and % 32 == 0, Cout % 128 == 0; persistent, 32 slots an XCD: ceil(tiles / 8) * (cout / 128)
# units must fill whole rounds of 32 to 80 %.  h8-512: the largest reference of the file (512 -> 512 on 10 x 50, 16 chunks).
CASES += [C("h8-m", "conv_h8_kernel<{A}>", MIN1, 128, 128, act=RELU, res=RB, batch=128),
          C("h8-r", "conv_h8_kernel<{A}>", RAG1, 96, 256, act=SILU, res=RA, batch=61, sl=True),
          C("h8-512", "conv_h8_kernel<{A}>", (10, 50), 512, 512, act=RELU, res=RN, batch=32),
          C("h8-leaky", "conv_h8_kernel<{A}>", MIN1, 128, 128, act=LEAKY, res=RA, batch=128),
          C("h8-none", "conv_h8_kernel<{A}>", MIN1, 128, 128, act=NONE, res=RN, batch=128)]
# ---- conv_pw_kernel<KS> / conv_pwx3_kernel<KS> (conv_pw.hip, conv_pw_x3.hip): 1x1, pad 0, stride 1 | 2, no residual, KS = ceil(cin / 32) in
# {1..6, 8, 10, 12, 16}; no batch condition.  -m: whole K steps; -r: the last step ragged (KS = 2: 40 channels), a Cout that is no multiple of 16.
# KS = 12, 16 with 256 outputs: the weights exceed the LDS budget and the output tiles are cut into ranges.
_PW_EPI = [(SILU, False), (RELU, False), (LEAKY, True), (NONE, False), (SILU, True)]
for i, ks in enumerate((1, 2, 3, 4, 5, 6, 8, 10, 12, 16)):
    (a1, f1), (a2, f2) = _PW_EPI[i % 5], _PW_EPI[(i + 2) % 5]
    s_m = 2 if ks in (4, 8) else 1
    CASES += [C("pw%d-m" % ks, "conv_pw{X}_kernel<%d>" % ks, PWM, 32 * ks, 256 if ks >= 12 else 64, k=1, s=s_m, act=a1, f32=f1, precs=P16 + PX3),
              C("pw%d-r" % ks, "conv_pw{X}_kernel<%d>" % ks, PWR, 32 * ks - 24, 40 if ks < 12 else (264 if ks == 12 else 248), k=1, s=2 if ks == 3 else 1, act=a2, f32=f2 and ks not in (2, 6, 12),
                sl=ks in (2, 6, 12), precs=P16 + PX3)]
# ---- conv_pwg_kernel<64 | 128> (conv_pwg.hip): 1x1 s1, Cin >= 128, whatever conv_pw does not take (K-step counts it is not instantiated for:
# 224 -> 7, 328 -> 11; a residual); <128>: ceil(pixels / 128) * ceil(cout / 128) >= 512
CASES += [C("pwg64-m", "conv_pwg_kernel<64>", PWM, 224, 64, k=1, act=SILU),
          C("pwg64-r", "conv_pwg_kernel<64>", PWR, 328, 72, k=1, act=LEAKY, sl=True),
          C("pwg64-res", "conv_pwg_kernel<64>", PWR, 128, 128, k=1, act=SILU, res=RA),
          C("pwg128-m", "conv_pwg_kernel<128>", PWM, 224, 512, k=1, act=RELU, res=RB, batch=70),
          C("pwg128-r", "conv_pwg_kernel<128>", PWR, 328, 488, k=1, act=NONE, batch=115)]
# ---- fc_kernel / fc_x3_kernel (conv_fc.hip, conv_pw_x3.hip): a 1x1 map.  Batches 1 and 17 (two row groups of 16); Cout 264: a ragged last tile;
# Cout 8200: the wide weight-streaming path of conv_fc.hip (cout > 8192)
CASES += [C("fc-1", "fc{X}_kernel", (1, 1), 256, 264, k=1, act=RELU, batch=1, precs=P16 + PX3),
          C("fc-17", "fc{X}_kernel", (1, 1), 256, 264, k=1, act=SILU, batch=17, precs=P16 + PX3),
          C("fc-17-f32", "fc{X}_kernel", (1, 1), 1000, 264, k=1, act=NONE, batch=17, f32=True, precs=P16 + PX3),
          C("fc-wide", "fc{X}_kernel", (1, 1), 64, 8200, k=1, act=LEAKY, batch=17, f32=True, precs=P16 + PX3)]
# ---- conv_stem_kernel / conv_stem_x3_kernel <kh, ceil(cout / 16), act> (conv_stem.hip, conv_stem_x3.hip): the first conv on its own, stride 2,
# reading the float32 frame (the input layer's conversion happens inside).  7x7: 64 outputs and ReLU in the split precision.
CASES += [C("stem3-m", "conv_stem{X}_kernel<3,1,{A}>", (32, 48), 3, 16, k=3, s=2, act=SILU, stem=True, precs=P16 + PX3),
          C("stem3-r", "conv_stem{X}_kernel<3,3,{A}>", (31, 45), 3, 48, k=3, s=2, act=LEAKY, stem=True, batch=5, precs=P16 + PX3),
          C("stem6-m", "conv_stem{X}_kernel<6,2,{A}>", (32, 48), 3, 32, k=6, s=2, pad=2, act=SILU, stem=True, precs=P16 + PX3),
          C("stem6-r", "conv_stem{X}_kernel<6,2,{A}>", (30, 46), 3, 32, k=6, s=2, pad=2, act=RELU, stem=True, batch=5, precs=P16 + PX3),
          C("stem7-m", "conv_stem{X}_kernel<7,4,{A}>", (32, 48), 3, 64, k=7, s=2, act=RELU, stem=True, precs=P16 + PX3),
          C("stem7-r", "conv_stem{X}_kernel<7,4,{A}>", (29, 43), 3, 64, k=7, s=2, act=RELU, stem=True, batch=5, precs=P16 + PX3)]
# ---- conv_igemm_kernel<in, out, BM, BN> (conv_kernels.hip): whatever nothing else takes -- here a 3x3 on 8 channels (conv_halo starts at 16) and
# a 5x5 on 24 -- and every conv of the fp32 mode.  pick_tile: BN = 16 | 32 | 64 by Cout (128 in the 16-bit modes for Cout % 128 == 0 or >= 256), BM = 128
# when ceil(pixels / 128) * ceil(cout / BN) >= 512 (240-pixel frames: 274 of them; 143-pixel ones: 459), else 64 (and BN 128 falls back to 64).
_IG_EPI = [(SILU, RN), (RELU, RB), (LEAKY, RA), (NONE, RN), (SILU, RA), (SILU, RB)]
for i, (bm, bn, cout, rcout) in enumerate(((64, 16, 16, 8), (64, 32, 32, 24), (64, 64, 64, 40), (128, 16, 16, 8), (128, 32, 32, 24), (128, 64, 64, 40))):
    (a1, r1), (a2, r2) = _IG_EPI[i], _IG_EPI[(i + 3) % 6]
    nm, nr = (3, 4) if bm == 64 else (274, 459)
    CASES += [C("ig%dx%d-m" % (bm, bn), "conv_igemm_kernel<{E},{O},%d,%d>" % (bm, bn), PWM, 8, cout, k=3, act=a1, res=r1, batch=nm, precs=P16 + P32),
              C("ig%dx%d-r" % (bm, bn), "conv_igemm_kernel<{E},{O},%d,%d>" % (bm, bn), PWR, 24, rcout, k=5, act=a2, res=r2, batch=nr, precs=P16 + P32),
              C("ig%dx%d-m-f32" % (bm, bn), "conv_igemm_kernel<{E},{O},%d,%d>" % (bm, bn), PWM, 8, cout, k=3, act=a2, res=RN, batch=nm, f32=True),
              C("ig%dx%d-r-f32" % (bm, bn), "conv_igemm_kernel<{E},{O},%d,%d>" % (bm, bn), PWR, 24, rcout, k=5, act=a1, res=RN, batch=nr, f32=True)]
CASES += [C("ig128x128-m", "conv_igemm_kernel<{E},{O},128,128>", PWM, 8, 256, k=3, act=SILU, res=RN, batch=137),
          C("ig128x128-r", "conv_igemm_kernel<{E},{O},128,128>", PWR, 24, 128, k=5, act=RELU, res=RA, batch=459),
          C("ig128x128-m-f32", "conv_igemm_kernel<{E},{O},128,128>", PWM, 8, 256, k=3, act=NONE, batch=137, f32=True),
          C("ig128x128-r-f32", "conv_igemm_kernel<{E},{O},128,128>", PWR, 24, 128, k=5, act=LEAKY, batch=459, f32=True),
          C("ig-1x1-res", "conv_igemm_kernel<{E},{O},64,64>", PWR, 40, 40, k=1, act=SILU, res=RA, precs=P16 + P32, sl=True),    # a 1x1 with a residual below conv_pwg's 128 channels
          C("ig-3x3-f32mode", "conv_igemm_kernel<{E},{O},64,64>", RAG1, 40, 56, k=3, act=SILU, res=RB, precs=P32, sl=True),    # fp32 mode: what conv_halo takes in the 16-bit modes
          C("ig-s2-f32mode", "conv_igemm_kernel<{E},{O},64,64>", RAG2, 96, 80, k=3, s=2, act=LEAKY, res=RA, precs=P32)]
# ---- fp16x3, 3x3 s1: conv_h8x3_kernel (conv_halo8_x3.hip): Cin >= 16, Cin * Cout >= half of the padded (32 | 64) product, and
# ceil(tiles / 8) * ceil(cout / 64) >= 12 (one round of an XCD's 32 slots at least 3 / 8 full)
CASES += [C("h8x3-m", "conv_h8x3_kernel<{A}>", MIN1, 64, 256, act=RELU, res=RB, batch=9, precs=PX3),
          C("h8x3-r", "conv_h8x3_kernel<{A}>", RAG1, 40, 120, act=SILU, res=RA, batch=22, precs=PX3, sl=True),
          C("h8x3-leaky", "conv_h8x3_kernel<{A}>", RAG1, 64, 64, act=LEAKY, res=RN, batch=46, precs=PX3),
          C("h8x3-none", "conv_h8x3_kernel<{A}>", MIN1, 32, 128, act=NONE, res=RA, batch=24, precs=PX3)]
# ---- fp16x3, 3x3 s2: conv_s2d_x3_kernel (conv_halo_s2.hip; window and weights by LDS-DMA): Cin % 32 == 0, 2 * Cout >= its 64-padding, no residual,
# frames * tiles256 * ceil(cout / 64) >= 96; conv_s2p_x3_kernel (register-staged) takes the layers s2d does not fit: more than 32 channel blocks
CASES += [C("s2d-m", "conv_s2d_x3_kernel<{A}>", MIN2, 64, 128, s=2, act=RELU, batch=48, precs=PX3),
          C("s2d-r", "conv_s2d_x3_kernel<{A}>", RAG2, 96, 72, s=2, act=SILU, batch=49, precs=PX3, sl=True),
          C("s2px3-m", "conv_s2p_x3_kernel<{A}>", MIN2, 32, 2112, s=2, act=LEAKY, batch=3, precs=PX3),
          C("s2px3-r", "conv_s2p_x3_kernel<{A}>", RAG2, 32, 2120, s=2, act=NONE, batch=4, precs=PX3),
          C("s2d-leaky", "conv_s2d_x3_kernel<{A}>", MIN2, 64, 128, s=2, act=LEAKY, batch=48, precs=PX3, sl=True),
          C("s2d-none", "conv_s2d_x3_kernel<{A}>", MIN2, 64, 128, s=2, act=NONE, batch=48, precs=PX3),
          C("s2px3-silu", "conv_s2p_x3_kernel<{A}>", MIN2, 32, 2112, s=2, act=SILU, batch=3, precs=PX3),
          C("s2px3-relu", "conv_s2p_x3_kernel<{A}>", MIN2, 32, 2112, s=2, act=RELU, batch=3, precs=PX3)]
# ---- fp16x3, the generic kernels (conv_x3.hip).  conv_x3_ksplit_kernel: Cout >= 32, at least 16 K steps of 32, fewer than 129 tiles of 64 x 64
# (ks-wide: Cout >= 64 and more than 320 tiles of 32 x 32 -> its 32 x 64 form).  conv_x3_igemm_kernel<BM, BN>: BN = 16 | 32 | 64 by Cout; BM 128 from
# 512 tiles of 128 rows on; else 64, 32 when the 64-row tiling has fewer than 128 tiles, then BN 64 -> 32 when the 32-row one has fewer too.
CASES += [C("ks-m", "conv_x3_ksplit_kernel", PWM, 64, 64, k=3, act=SILU, res=RA, precs=PX3),
          C("ks-r", "conv_x3_ksplit_kernel", (7, 9), 24, 40, k=5, act=LEAKY, res=RB, precs=PX3, sl=True),
          C("ks-s2", "conv_x3_ksplit_kernel", RAG2, 72, 200, k=3, s=2, act=RELU, res=RA, precs=PX3),
          C("ks-wide", "conv_x3_ksplit_kernel", PWM, 64, 128, k=3, act=NONE, res=RN, batch=12, precs=PX3),
          C("ksf-m", "conv_x3_ksplit_kernel<f32>", PWM, 64, 64, k=3, act=NONE, f32=True, precs=PX3),
          C("ksf-r", "conv_x3_ksplit_kernel<f32>", (7, 9), 24, 40, k=5, act=SILU, f32=True, precs=PX3)]
for i, (bm, bn, cout, rcout, nm, nr) in enumerate(((64, 16, 16, 8, 3, 4), (128, 16, 16, 8, 274, 459), (32, 32, 32, 24, 3, 4), (64, 32, 32, 24, 34, 57),
                                                  (128, 32, 32, 24, 274, 459), (32, 64, 64, 40, 20, 33), (64, 64, 64, 40, 34, 57), (128, 64, 64, 40, 274, 459))):
    (a1, r1), (a2, r2) = _IG_EPI[i % 6], _IG_EPI[(i + 3) % 6]
    CASES += [C("x3ig%dx%d-m" % (bm, bn), "conv_x3_igemm_kernel<%d,%d>" % (bm, bn), PWM, 8, cout, k=3, act=a1, res=r1, batch=nm, precs=PX3),
              C("x3ig%dx%d-r" % (bm, bn), "conv_x3_igemm_kernel<%d,%d>" % (bm, bn), PWR, 8, rcout, k=5, act=a2, res=r2, batch=nr, precs=PX3, sl=i % 2 == 1),
              C("x3ig%dx%d-m-f32" % (bm, bn), "conv_x3_igemm_kernel<%d,%d,f32>" % (bm, bn), PWM, 8, cout, k=3, act=a2, batch=nm, f32=True, precs=PX3),
              C("x3ig%dx%d-r-f32" % (bm, bn), "conv_x3_igemm_kernel<%d,%d,f32>" % (bm, bn), PWR, 8, rcout, k=5, act=a1, batch=nr, f32=True, precs=PX3)]
assert len({c["id"] for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------------- the run
def build_graph(c):
    """The unit graph of a case.  Returns (graph, weights, names to fetch, name of the layer in front of the conv or None for a stem)."""
    H, W = c["hw"]
    ws = M.SynthWeights(17, gain=1.0)
    g = M.Graph("convunit", 3, H, W, ws)
    x, c3 = g.input()
    k, s, p = c["k"], c["s"], c["pad"]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    fetch = ["test"]
    if c["stem"]:
        a = x
    else:
        full = g.conv(x, c["cin"] + 16 if c["sl"] else c["cin"], 1, 1, "expand", act=NONE, true_cin=c3)
        a = full.slice(8, c["cin"]) if c["sl"] else full
        fetch.append("expand")
    res = None
    if c["res"] != RN:
        if (Ho, Wo) != (H, W) or c["cout"] != c["cin"]:     # another shape: a second conv fed by the graph input
            res = g.conv(x, c["cout"], 1, s, "resid", act=NONE, true_cin=c3, pad=0)
            assert (res.h, res.w) == (Ho, Wo)
            fetch.append("resid")
        else:
            res = a
    cat = out = None
    if c["sl"]:
        assert not c["f32"]
        cat, out = _guarded(g, x, c3, Ho, Wo, c["cout"], geom=(1, s, 0))
        fetch += ["guard_lo", "guard_hi"]
    y = g.conv(a, c["cout"], k, s, "test", act=c["act"], res=res, res_mode=c["res"], f32_out=c["f32"], out=out, pad=p,
               true_cin=c3 if c["stem"] else None)
    if c["f32"]:
        g.output(y, 0, [1, y.h * y.w * c["cout"]], "o")
    else:
        z = g.conv(cat if c["sl"] else y, 8, 1, 1, "tap", act=NONE, f32_out=True)
        g.output(z, 0, [1, z.h * z.w * 8], "o")
    return g, ws, fetch


def distinct(c):
    """How many frames of the batch are distinct: all of them where the two float64 convs of the reference stay inside REF_FLOPS, else as
    many as do (3 at least), an odd number so that the period of the repetition shares no factor with the 8-tile groups and 32-slot rounds
    the persistent kernels walk.  Frame k of the batch is frame k % distinct(c)."""
    H, W = c["hw"]
    k, s, p = c["k"], c["s"], c["pad"]
    per_frame = 4.0 * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1) * c["cout"] * c["cin"] * k * k
    d = min(c["batch"], max(DISTINCT, int(REF_FLOPS // per_frame)))
    return d if d == c["batch"] or d % 2 == 1 else d - 1


def frames(c):
    """distinct(c) signed frames, repeated over the batch."""
    H, W = c["hw"]
    d = distinct(c)
    f = np.random.default_rng(5).uniform(-1, 1, (d, 3, H, W)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([f] * ((c["batch"] + d - 1) // d), 0)[:c["batch"]])


def expected_label(c, prec):
    """{A}: the activation; {E}: the element type; {O}: the output's (float32 for f32_out and in fp32 mode); {X}: _x3 in the split precision."""
    e = ELEM_TAG.get(prec, "")
    return (c["label"].replace("{A}", ACT_TAG[c["act"]]).replace("{O}", "f32" if c["f32"] or prec == "fp32" else e).replace("{E}", e)
            .replace("pw{X}", "pwx3" if prec == "fp16x3" else "pw").replace("{X}", "_x3" if prec == "fp16x3" else ""))


def run_engine(tmp_path, c, prec):
    g, ws, fetch = build_graph(c)
    path = str(tmp_path / "convunit.hipm")
    g.save(path)
    xin = frames(c)
    e = CE.HipEngine(path, prec, c["batch"])
    try:
        label = e.layer_kernel(e.layer_index("test"), c["batch"])
        assert label == expected_label(c, prec), "%s %s: resolves to %s, the case is written for %s" % (c["id"], prec, label, expected_label(c, prec))
        e.engine_inference(xin)
        # the output (and the guards) of every frame; the inputs of the distinct frames only: they are what the reference is applied to
        acts = {n: e.fetch_activation(n, c["batch"] if n in ("test", "guard_lo", "guard_hi") else distinct(c)) for n in fetch}
    finally:
        e.close()
    return ws, xin, acts, label


def check_case(tmp_path, c, prec):
    ws, xin, acts, label = run_engine(tmp_path, c, prec)
    n3 = distinct(c)
    for nm, a in acts.items():                      # every copy of a frame is the frame: the reference is computed for the distinct ones
        for kf in range(n3, a.shape[0]):
            assert np.array_equal(a[kf], a[kf % n3]), "%s %s: %s of frame %d differs from frame %d's" % (c["id"], prec, nm, kf, kf % n3)
    got = acts["test"]
    if c["stem"]:
        x = R.storage_round(xin[:n3], prec)          # conv_stem*.hip converts the frame itself: pack2 / x3_split, round to nearest even
    else:
        x = acts["expand"][:n3, 8:8 + c["cin"]] if c["sl"] else acts["expand"][:n3]
    assert (x > 0).mean() > 0.2 and (x < 0).mean() > 0.2 and np.abs(x).max() < 1e3, "signed inputs"
    r = None
    if c["res"] != RN:
        r = acts["resid"][:n3] if "resid" in acts else x
    w = CR.weights_as_stored(ws.store["test.weight"], prec)
    b = ws.store["test.bias"]
    want, S, v = CR.conv_layer_ref(x, w, b, c["s"], c["pad"], c["act"], r, c["res"])
    assert got.shape == (c["batch"],) + want.shape[1:], (got.shape, want.shape)
    assert np.abs(want).max() < 6000.0, "far from the half range: saturation has its own test"
    yard, yt, ys = CR.conv_yardstick(x, w, b, c["s"], c["pad"], c["act"], r, c["res"], want, S)
    slack = CR.conv_slack(x, w, c["s"], c["pad"], c["act"], prec, S, v)
    ok, worst, err = CR.check(got[:n3], want, prec, slack, c["f32"])
    print("%s %s %s: worst |err| / bound %.3f (|err| %.3e)  yardstick ratio %.3f (torch %.3f, sequential %.3f)  batch %d (%d distinct)"
          % (c["id"], prec, label, worst, err, yard, yt, ys, c["batch"], n3))
    assert yard <= CR.YARD_CONV, (yard, CR.YARD_CONV)
    assert ok.all(), (int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), got[:n3][~ok][:4], want[~ok][:4])
    if c["sl"]:
        _check_guards(acts, got, np.concatenate([want] * ((c["batch"] + n3 - 1) // n3), 0)[:c["batch"]], prec)


PARAMS = [pytest.param(c, prec, id="%s-%s" % (c["id"], prec)) for c in CASES for prec in c["precs"]]


@pytest.mark.parametrize("c,prec", PARAMS)
def test_conv_layer_per_element(tmp_path, c, prec):
    check_case(tmp_path, c, prec)
