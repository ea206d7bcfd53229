"""GPU: every FUSED conv launch, element by element against float64 (tests/fused_ref.py on top of tests/conv_ref.py).  The tensor between
the fused convs never reaches memory, so it is computed: in float64 from the launch's fetched INPUT, rounded as the kernel stores it, and
the ways the device's rounding may differ from the reference's widen the bound of the elements that read it (the ambiguity form; no
element is exempted, nothing read off the device enters a bound).  tests/test_fused_ref_cpu.py judges that checker first.

Pattern: input (signed uniform(-1, 1) frames, all distinct) -> 1x1 "expand" with no activation (signed values) -> the fused launch -> 1x1
fp32 "tap"; a stem reads the input layer (the fp32 frame, which conv_stem*.hip rounds itself: storage_round).  The launch's input is
fetched and is the reference's operand; weights are rounded with weights_as_stored.  The kernel label and the "(fused into ...)" labels
of the absorbed layers are asserted.  Where a batch is needed only to make persistent workgroups walk several tiles, a few frames are
distinct and repeat with an odd period: every copy must equal its original bit for bit, the reference covers the distinct ones.  Slice
cases write between guard channels set to 7.0 in front of the launch (test_gpu_ops_exact.py's _guarded / _check_guards; the pair's output
offset of 20 needs 20-channel guards, written by one zero-weight conv over the whole buffer).

Two kinds of case per kernel.  CHAIN: random SynthWeights, the chained bound.  PROBE: a later stage is a signed selection (+-1 on one
(tap, channel) per output channel, bias 0, exact in every storage type), so the output is round(act(+-t_dev)) [+ shortcut] and the
EARLIER stage is seen element by element to R(want) + L (R(t64) + slack1) + A, the out-of-image halo included: a probe on tap (0, 0)
reads intermediate row -1 at output row 0, which must be exactly zero.  Between the probe cases of a kernel every tap and every
intermediate channel is read.

label -> cases
  conv_pair_kernel<16|32>                     pair<C>-16x16 / -13x37 / -33x17 (with and without shortcut between them), pair<C>-slice (input at channel 8 of
                                              a wider buffer, output at channel 20: a multiple of 4, not of 8), pair<C>-probe (conv B a selection)        fp16, bf16
  conv_c2f16_kernel, conv_c2f16_x3_kernel     c2f-16x16 / -13x37 / -33x17, c2f-slice (guarded output), c2f-probe-cv2-lo / -hi (cv2 a selection over concat
                                              channels 0..31 / 16..47: y0, y1, y2), c2f-probe-B (conv B and cv2 selections: conv A's zeroed 18 x 18 region),
                                              c2f-probe-cv1 / -cv1-cv2 (cv1 a selection: the Bottleneck reads a tensor with next to no ambiguity, so conv A and
                                              conv B are seen as sharply as a bare pair's, through a random cv2 and through a selection over y1, y2);
                                              x3: c2f-persist (64 frames of 33 x 17 = 384 tiles on 256 workgroups: second tile, next-window prefetch)
  conv_stem_kernel<3|6,1,SILU>+conv3x3s2,     stem2-* : 64x96 (whole 8 x 16 tiles), 62x90 (odd stem extents: the second conv's last row and column are padding),
  conv_stem2_x3_kernel<3|6>+conv3x3s2         18x20 (under one tile); pads 0 .. kh / 2, 1 - 3 input channels; stem2-persist (more tiles than the persistent
                                              grid: 768 / 256 x ADAS_STEM2_X3_WGS workgroups); stem2-probe (the second conv a selection over 16 channels x 9 taps)
  conv_stem_kernel<7,4,RELU>+pool             pool-*: the nine STEM_POOL shapes of tests/test_gpu_x3_stems.py, interval bound                              fp16, bf16
  conv_h8_kernel<RELU>+shortcut               h8ds-m (16 x 32, Cp 64 -> C 128, batch 128), h8ds-r (13 x 37 from 25 x 73, Cp 96 -> C 256, batch 61), h8ds-32 (Cp 32)    fp16, bf16

Out of scope: the fused Detect kernels (tests/test_gpu_detect_exact.py: every anchor against float64, bound in tests/detect_ref.py);
conv_ml / grouped launches (bit-identical to the per-layer launches by tests/test_gpu_ml.py); the folded upsample (bit-identical to the
unfolded conv, which tests/test_gpu_conv_exact.py covers per element); the fp16x3 stem + pool (bit-identical to its per-element-tested
two-launch form by tests/test_gpu_x3_stems.py)."""
import importlib

import numpy as np
import pytest

import conv_ref as CR
import fused_ref as FR
import ops_ref as R
from conftest import load_pkg
from test_gpu_ops_exact import _check_guards, _guarded
from test_gpu_x3_stems import STEM_POOL

pytestmark = pytest.mark.gpu
load_pkg()
CE = importlib.import_module("adas_amd.coreEngine")
M = importlib.import_module("adas_amd.models")

assert (M.ACT_NONE, M.ACT_SILU, M.ACT_RELU, M.ACT_LEAKY) == (R.ACT_NONE, R.ACT_SILU, R.ACT_RELU, R.ACT_LEAKY)
assert (M.RES_NONE, M.RES_AFTER_ACT, M.RES_BEFORE_ACT) == (CR.RES_NONE, CR.RES_AFTER_ACT, CR.RES_BEFORE_ACT)
NONE, SILU, RELU = R.ACT_NONE, R.ACT_SILU, R.ACT_RELU
P16, P3 = ("fp16", "bf16"), ("fp16", "bf16", "fp16x3")
MAPS = ((16, 16), (13, 37), (33, 17))      # one tile;  H below a tile, last tile 5 wide;  one-pixel remainders both ways, 6 tiles
IN_PAIR, IN_C2F, IN_STEM, IN_SHORTCUT = "(fused into the pair launch)", "(fused into the C2f launch)", "(fused into the stem launch)", "(fused into the conv it is the shortcut of)"
GUARD_OFF = 20                             # the pair's slice case: 20 guard channels | C | 20 guard channels


def frames(batch, distinct, c, hw, seed=5):
    """`distinct` signed frames, repeated over the batch (frame k is frame k % distinct)."""
    f = np.random.default_rng(seed).uniform(-1, 1, (distinct, c) + tuple(hw)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([f] * ((batch + distinct - 1) // distinct), 0)[:batch])


def run(tmp_path, g, prec, xin, labels, fetch, distinct):
    """One engine: asserts the labels, runs the batch, fetches `fetch` = {name: frames to fetch}; the copies of a frame equal the frame."""
    path = str(tmp_path / "fusedunit.hipm")
    g.save(path)
    batch = xin.shape[0]
    e = CE.HipEngine(path, prec, batch)
    try:
        for name, want in labels.items():
            got = e.layer_kernel(e.layer_index(name), batch)
            assert got == want, "%s resolves to %s, the case is written for %s" % (name, got, want)
        e.engine_inference(xin)
        acts = {n: e.fetch_activation(n, k) for n, k in fetch.items()}
    finally:
        e.close()
    for nm, a in acts.items():
        for kf in range(distinct, a.shape[0]):
            assert np.array_equal(a[kf], a[kf % distinct]), "%s of frame %d differs from frame %d's" % (nm, kf, kf % distinct)
    return acts


def signed(x):
    assert (x > 0).mean() > 0.2 and (x < 0).mean() > 0.2 and np.abs(x).max() < 1e3, "signed inputs"


def report(cid, prec, label, final, stages, got, batch, distinct):
    """Prints the case's figures, then asserts: every stage's yardstick ratio inside the recorded constant, every element inside its bound."""
    ok, worst, err = final.check(got)
    chain = [s for s in stages if s.yard[0] > 0]
    amb = [float(s.stored()[2].mean()) for s in stages[:-1]]
    print("%s %s %s: worst |err| / bound %.3f (|err| %.3e)  yardstick ratios %s  ambiguous %s  chained term median %.2f R(want)  batch %d (%d distinct)"
          % (cid, prec, label, worst, err, " ".join("%.3f" % s.yard[0] for s in chain), " ".join("%.1f%%" % (100 * a) for a in amb),
             float(np.median(final.chain / np.maximum(R.store_bound(final.want, prec), 1e-300))), batch, distinct))
    for s in chain:
        assert s.yard[0] <= CR.YARD_CONV, (s.yard, CR.YARD_CONV)
    assert np.abs(final.want).max() < 6000.0, "far from the half range: saturation has its own test"
    bad = np.argwhere(~ok)
    assert ok.all(), (int((~ok).sum()), "frame, channel, y, x:", bad[:6].tolist(), "rows", sorted(set(bad[:, 2].tolist()))[:12], "columns", sorted(set(bad[:, 3].tolist()))[:12],
                      "channels", sorted(set(bad[:, 1].tolist()))[:12], got[~ok][:4], final.want[~ok][:4])


def with_weights(build, override):
    """The graph built twice: once on SynthWeights (every parameter drawn), once on a DictWeights copy with `override` applied."""
    ws = M.SynthWeights(17, gain=1.0)
    g = build(ws)
    if not override:
        return g, ws.store
    d = {k: v.copy() for k, v in ws.store.items()}
    for k, v in override.items():
        assert d[k].shape == v.shape, (k, d[k].shape, v.shape)
        d[k] = v.astype(np.float32)
    return build(M.DictWeights(d)), d


def stored_w(store, name, prec):
    return CR.weights_as_stored(store[name + ".weight"], prec), store[name + ".bias"]


def sel(cout, cin):
    """3x3 selection: output channel o reads tap o % 9 of channel o % cin, sign alternating -- every tap and every channel (cout >= 9, cin)."""
    return FR.selection(cout, cin, 3, [(o % 9, o % cin) for o in range(cout)])


def sel_cat(ch0):
    """cv2 of the C2f block as a selection: output channel o reads concat channel ch0 + o (of 48), sign alternating."""
    return FR.selection(32, 48, 1, [(0, ch0 + o) for o in range(32)])


# ------------------------------------------------------------------------------------------------------------------------- conv_pair
PAIR = []
for C_ in (16, 32):
    for i, hw in enumerate(MAPS):
        PAIR.append(dict(id="pair%d-%dx%d" % ((C_,) + hw), c=C_, hw=hw, sc=(i + C_ // 16) % 2 == 0, sl=False, probe=False))
    PAIR += [dict(id="pair%d-slice" % C_, c=C_, hw=MAPS[1], sc=True, sl=True, probe=False), dict(id="pair%d-probe" % C_, c=C_, hw=MAPS[2], sc=True, sl=False, probe=True)]


@pytest.mark.parametrize("prec", P16)
@pytest.mark.parametrize("c", PAIR, ids=lambda c: c["id"])
def test_conv_pair(tmp_path, c, prec):
    """A bare pair: expand -> 3x3 SiLU -> 3x3 SiLU [+ shortcut]; nothing conv_c2f would take (no concat buffer around it)."""
    C_, (H, W) = c["c"], c["hw"]

    def build(ws):
        g = M.Graph("pairunit", 3, H, W, ws)
        x, c3 = g.input()
        full = g.conv(x, C_ + 16 if c["sl"] else C_, 1, 1, "expand", act=NONE, true_cin=c3)
        a = full.slice(8, C_) if c["sl"] else full
        out = cat = None
        if c["sl"]:      # one zero-weight conv with bias 7.0 fills the whole buffer in front of the pair
            cat = g.conv(x, C_ + 2 * GUARD_OFF, 1, 1, "guards", act=NONE, true_cin=c3, weight=np.zeros((C_ + 2 * GUARD_OFF, c3, 1, 1), np.float32), bias_fill=7.0)
            out = cat.slice(GUARD_OFF, C_)
        t = g.conv(a, C_, 3, 1, "A")
        y = g.conv(t, C_, 3, 1, "B", out=out, res=a if c["sc"] else None, res_mode=M.RES_AFTER_ACT if c["sc"] else M.RES_NONE)
        z = g.conv(cat if c["sl"] else y, 8, 1, 1, "tap", act=NONE, f32_out=True)
        g.output(z, 0, [1, z.h * z.w * 8], "o")
        return g

    g, store = with_weights(build, {"B.weight": sel(C_, C_), "B.bias": np.zeros(C_)} if c["probe"] else None)
    xin = frames(3, 3, 3, (H, W))
    fetch = {"expand": 3, "B": 3}
    if c["sl"]:
        fetch["guards"] = 3
    label = "conv_pair_kernel<%d>" % C_
    acts = run(tmp_path, g, prec, xin, {"A": label, "B": IN_PAIR}, fetch, 3)
    x = acts["expand"][:, 8:8 + C_] if c["sl"] else acts["expand"]
    signed(x)
    (wa, ba), (wb, bb) = stored_w(store, "A", prec), stored_w(store, "B", prec)
    A, B = FR.pair_ref(x, wa, ba, wb, bb, prec, c["sc"], probe=c["probe"])
    report(c["id"], prec, label, B, (A, B), acts["B"], 3, 3)
    if c["sl"]:
        gd = acts["guards"]
        assert (gd[:, :GUARD_OFF] == 7.0).all() and (gd[:, GUARD_OFF + C_:] == 7.0).all(), "guard channels overwritten"
        assert np.array_equal(gd[:, GUARD_OFF:GUARD_OFF + C_], acts["B"])


# ------------------------------------------------------------------------------------------------------------------------- conv_c2f16
C2F = [dict(id="c2f-%dx%d" % hw, hw=hw, probe=(), sl=False, batch=3, precs=P3) for hw in MAPS]
C2F += [dict(id="c2f-slice", hw=MAPS[1], probe=(), sl=True, batch=3, precs=P3),
        dict(id="c2f-probe-cv2-lo", hw=MAPS[2], probe=("cv2",), ch0=0, sl=False, batch=3, precs=P3),
        dict(id="c2f-probe-cv2-hi", hw=MAPS[1], probe=("cv2",), ch0=16, sl=False, batch=3, precs=P3),
        dict(id="c2f-probe-B", hw=MAPS[2], probe=("B", "cv2"), ch0=16, sl=False, batch=3, precs=P3),
        dict(id="c2f-probe-cv1", hw=MAPS[1], probe=("cv1",), sl=False, batch=3, precs=P3),
        dict(id="c2f-probe-cv1-cv2", hw=MAPS[2], probe=("cv1", "cv2"), ch0=16, sl=False, batch=3, precs=P3),
        dict(id="c2f-persist", hw=MAPS[2], probe=(), sl=False, batch=64, precs=("fp16x3",))]
C2F_NAMES = ("blk.cv1.conv", "blk.m.0.cv1.conv", "blk.m.0.cv2.conv", "blk.cv2.conv")


@pytest.mark.parametrize("c,prec", [pytest.param(c, p, id="%s-%s" % (c["id"], p)) for c in C2F for p in c["precs"]])
def test_conv_c2f16(tmp_path, c, prec):
    """models._c2f(g, a, 32, 1, True): cv1 -> (y0, y1) -> conv A -> conv B + y1 -> cv2 over the concat, one launch."""
    H, W = c["hw"]

    def build(ws):
        g = M.Graph("c2funit", 3, H, W, ws)
        x, c3 = g.input()
        a = g.conv(x, 32, 1, 1, "expand", act=NONE, true_cin=c3)
        cat = out = None
        if c["sl"]:
            cat, out = _guarded(g, x, c3, H, W, 32)
        y = M._c2f(g, a, 32, 1, True, "blk", out=out)
        z = g.conv(cat if c["sl"] else y, 8, 1, 1, "tap", act=NONE, f32_out=True)
        g.output(z, 0, [1, z.h * z.w * 8], "o")
        return g

    over = {}
    if "cv1" in c["probe"]:      # y = SiLU(+-x), channel by channel: the Bottleneck's input is a rounding of the fetched tensor alone
        over.update({"blk.cv1.conv.weight": FR.selection(32, 32, 1, [(0, o) for o in range(32)]), "blk.cv1.conv.bias": np.zeros(32)})
    if "B" in c["probe"]:
        over.update({"blk.m.0.cv2.conv.weight": sel(16, 16), "blk.m.0.cv2.conv.bias": np.zeros(16)})
    if "cv2" in c["probe"]:      # 32 outputs over the 32 concat channels from ch0 on
        over.update({"blk.cv2.conv.weight": sel_cat(c["ch0"]), "blk.cv2.conv.bias": np.zeros(32)})
    g, store = with_weights(build, over)
    batch, d = c["batch"], 3
    xin = frames(batch, d, 3, (H, W))
    fetch = {"expand": d, "blk.cv2.conv": batch}
    if c["sl"]:
        fetch.update(guard_lo=batch, guard_hi=batch)
    label = "conv_c2f16_x3_kernel" if prec == "fp16x3" else "conv_c2f16_kernel"
    labels = {n: IN_C2F for n in C2F_NAMES[1:]}
    labels[C2F_NAMES[0]] = label
    acts = run(tmp_path, g, prec, xin, labels, fetch, d)
    x = acts["expand"]
    signed(x)
    wb = [stored_w(store, n, prec) for n in C2F_NAMES]
    stages = FR.c2f_ref(x, [w for w, _ in wb], [b for _, b in wb], prec, probe=c["probe"])
    got = acts["blk.cv2.conv"]
    report(c["id"], prec, label, stages[-1], stages, got[:d], batch, d)
    if c["sl"]:
        _check_guards(acts, got, stages[-1].want, prec)


# ------------------------------------------------------------------------------------------------------------------------- stem + second conv
#         id              H   W  cin kh pad batch distinct probe
STEM2 = [("stem2-64x96", 64, 96, 3, 3, 1, 3, 3, False), ("stem2-62x90", 62, 90, 3, 6, 2, 3, 3, False), ("stem2-18x20", 18, 20, 1, 3, 0, 3, 3, False),
         ("stem2-62x90-k3", 62, 90, 2, 3, 1, 3, 3, False), ("stem2-64x96-k6p0", 64, 96, 1, 6, 0, 3, 3, False), ("stem2-62x90-k6p1", 62, 90, 3, 6, 1, 3, 3, False),
         ("stem2-18x20-k6p3", 18, 20, 2, 6, 3, 3, 3, False),
         ("stem2-persist", 18, 20, 3, 3, 1, 800, 5, False),        # one 8 x 16 tile a frame: 800 tiles on 768 (16-bit) / 512 (fp16x3) workgroups
         ("stem2-probe", 62, 90, 3, 3, 1, 3, 3, True)]


@pytest.mark.parametrize("prec", P3)
@pytest.mark.parametrize("c", STEM2, ids=lambda c: c[0])
def test_stem_with_second_conv(tmp_path, c, prec):
    """fp32 frame -> k x k s2 SiLU stem on 16 channels (kept in LDS) -> 3x3 s2 p1 SiLU on 32 channels."""
    cid, H, W, cin, kh, pad, batch, d, probe = c

    def build(ws):
        g = M.Graph("stem2unit", cin, H, W, ws)
        x, ct = g.input()
        s = g.conv(x, 16, kh, 2, "stem", act=SILU, true_cin=ct, pad=pad)
        y = g.conv(s, 32, 3, 2, "conv2", act=SILU)
        z = g.conv(y, 8, 1, 1, "tap", act=NONE, f32_out=True)
        g.output(z, 0, [1, z.h * z.w * 8], "o")
        return g

    g, store = with_weights(build, {"conv2.weight": sel(32, 16), "conv2.bias": np.zeros(32)} if probe else None)
    xin = frames(batch, d, cin, (H, W))
    label = ("conv_stem2_x3_kernel<%d>+conv3x3s2" if prec == "fp16x3" else "conv_stem_kernel<%d,1,SILU>+conv3x3s2") % kh
    acts = run(tmp_path, g, prec, xin, {"input": IN_STEM, "stem": label, "conv2": IN_STEM}, {"conv2": batch}, d)
    x = R.storage_round(xin[:d], prec)          # conv_stem*.hip converts the frame itself: pack2 / x3_split, round to nearest even
    (w1, b1), (w2, b2) = stored_w(store, "stem", prec), stored_w(store, "conv2", prec)
    s1, s2 = FR.stem2_ref(x, w1, b1, pad, w2, b2, prec, probe=probe)
    report(cid, prec, label, s2, (s1, s2), acts["conv2"][:d], batch, d)


# ------------------------------------------------------------------------------------------------------------------------- stem + max-pool
@pytest.mark.parametrize("prec", P16)
@pytest.mark.parametrize("case", STEM_POOL, ids=str)
def test_stem_with_pool(tmp_path, case, prec):
    """7x7 s2 ReLU stem on 64 channels with the 3x3 s2 p1 max-pool in its launch: rounding and the maximum are monotone, so every pooled
    element lies in [maxpool(want - b), maxpool(want + b)], b = R(want) + slack of the conv's elements (-inf padding: a conv pixel past an
    odd conv extent must not enter the window)."""
    H, W, cin, pad, batch, coff = case
    ws = M.SynthWeights(17, gain=1.0)
    g = M.Graph("stempoolunit", cin, H, W, ws)
    x, ct = g.input()
    s = g.conv(x, 64, 7, 2, "stem", act=RELU, true_cin=ct, pad=pad)
    hp, wp = (s.h - 1) // 2 + 1, (s.w - 1) // 2 + 1
    slot = None if coff is None else g.buf(hp, wp, 80).slice(coff, 64)
    y = g.maxpool(s, 3, 2, 1, out=slot, name="pool")
    z = g.conv(y, 8, 1, 1, "tap", act=NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    xin = frames(batch, batch, cin, (H, W), seed=3)
    label = "conv_stem_kernel<7,4,RELU>+pool"
    acts = run(tmp_path, g, prec, xin, {"input": IN_STEM, "stem": label, "pool": IN_STEM}, {"pool": batch}, batch)
    w1, b1 = stored_w(ws.store, "stem", prec)
    st = FR.stage(R.storage_round(xin, prec), w1, b1, 2, pad, RELU, prec)
    lo, hi = FR.pool_interval(st)
    got = acts["pool"]
    assert got.shape == lo.shape, (got.shape, lo.shape)
    ok, out = FR.pool_check(got, lo, hi)
    mid = R.maxpool_ref(st.want, 3, 2, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(got == mid, 0.0, np.abs(got - mid) / np.maximum(hi - mid, mid - lo))))
    print("pool-%s %s %s: worst |got - maxpool(want)| / interval half width %.3f  yardstick ratio %.3f  batch %d (%d distinct)" % (case, prec, label, worst, st.yard[0], batch, batch))
    assert st.yard[0] <= CR.YARD_CONV, (st.yard, CR.YARD_CONV)
    assert (mid > 0).mean() > 0.3, "the pooled map is not all ReLU zeros"
    bad = np.argwhere(~ok)
    assert ok.all(), (int((~ok).sum()), bad[:6].tolist(), "rows", sorted(set(bad[:, 2].tolist()))[:12], "columns", sorted(set(bad[:, 3].tolist()))[:12], got[~ok][:4], lo[~ok][:4], hi[~ok][:4])


# ------------------------------------------------------------------------------------------------------------------------- conv_h8 + shortcut
#        id        block output  Cp   C   batch
H8DS = [("h8ds-m", (16, 32), 64, 128, 128), ("h8ds-r", (13, 37), 96, 256, 61), ("h8ds-32", (16, 32), 32, 128, 128)]


@pytest.mark.parametrize("prec", P16)
@pytest.mark.parametrize("c", H8DS, ids=lambda c: c[0])
def test_projection_shortcut_in_conv_h8(tmp_path, c, prec):
    """ResNet layerN.0: out = relu(conv3x3(t) + b + conv1x1_s2(x) + b_d), the projection accumulated in the 3x3's fp32 accumulator: one
    expression, no stored stage.  conv1 (t) and expand (x) are fetched."""
    cid, (H, W), cp, C_, batch = c
    Hin, Win = 2 * H - (H % 2), 2 * W - (W % 2)
    ws = M.SynthWeights(17, gain=1.0)
    g = M.Graph("dsunit", 3, Hin, Win, ws)
    x0, c3 = g.input()
    x = g.conv(x0, cp, 1, 1, "expand", act=NONE, true_cin=c3)
    t = g.conv(x, C_, 3, 2, "conv1", act=RELU)
    dn = g.conv(x, C_, 1, 2, "down", act=NONE, pad=0)
    y = g.conv(t, C_, 3, 1, "conv2", act=RELU, res=dn, res_mode=M.RES_BEFORE_ACT)
    z = g.conv(y, 8, 1, 1, "tap", act=NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    assert (y.h, y.w) == (H, W)
    d = 3
    xin = frames(batch, d, 3, (Hin, Win))
    label = "conv_h8_kernel<RELU>+shortcut"
    acts = run(tmp_path, g, prec, xin, {"conv2": label, "down": IN_SHORTCUT}, {"expand": d, "conv1": d, "conv2": batch}, d)
    signed(acts["expand"])
    (w2, b2), (wd, bd) = stored_w(ws.store, "conv2", prec), stored_w(ws.store, "down", prec)
    st = FR.folded_ref(acts["conv1"], w2, b2, acts["expand"], wd, bd, RELU, prec)
    assert (st.want > 0).mean() > 0.2
    report(cid, prec, label, st, (st,), acts["conv2"][:d], batch, d)
