"""GPU: the Detect head kernels, every element of the (B, 4 + nc, A) head against float64 (tests/detect_ref.py on top of
tests/conv_ref.py; tests/test_detect_ref_cpu.py judges that checker first, and plans every graph of this file on the CPU).

Pattern: input (signed uniform(-1, 1) frames, all distinct, batch 3) -> 1x1 "expand" with no activation = P3 -> 3x3 s2 SiLU = P4 -> 3x3 s2
SiLU = P5; per level SiLU 1x1 convs to the hidden widths cb / cc ("hb<i>", "hc<i>"), 1x1 float32 convs without activation to 64 box
logits and nc class logits ("box<i>", "cls<i>"), OP_DETECT_V8 with strides 8 / 16 / 32.  The fused kernels' operands are the fetched
hidden maps and the weights as stored (conv_ref.weights_as_stored); detect_v8_kernel's are the fetched float32 logits.  The kernel label
and the six "(fused into the Detect launch)" labels are asserted.

Geometries   G1  9x13 / 5x7 / 3x4  = 117 (one full 64-anchor block + 53) / 35 / 12 cells, A = 164: ragged tails on every level
             G2  16x16 / 8x8 / 4x4 = 256 / 64 / 16, A = 336: level boundaries on block boundaries, one level exactly one block
Widths (cb, cc, nc)   (64, 80, 80) YOLOv8n's: the last class K step half empty, detect_v8_kernel's second 64-class chunk 16 wide;
             (96, 40, 24) three box K steps, lane group 0 alone in the second class K step, the second class tile half full;
             (32, 32, 8) one half-empty class tile;  (64, 64, 20) nc % 8 != 0: the second class tile a quarter full (the float32 logits
             need nc % 4 == 0 to be conv_pw's, in the split precision too -- pw_applicable / pw_x3_applicable -- so this head fuses in all
             three modes; (64, 64, 22) fuses in none: planned on the CPU).  Every width on G1, the first two on G2.
Stress       box-conv weights x 40, bias linspace(-60, 60): |box logit| >= 100 through every DFL softmax, all four precisions.
Sink         SINK = true launches (what every pipeline step runs) into guarded buffers: bit-identical box rows, conf / cls bit-identical to
             max / first arg-max of the rows of the run without the sink (checked against float64 just before), and independently inside the
             float64 bound / admissible set.  Tie cases: classes 3, 19, 40 (one lane, three tiles; 40 in another lane) and 14, 17 (lane
             group 3 of tile 0, lane group 0 of tile 1) get identical weight rows and a raised bias: cls must be the smallest of the group.
v5 sink      detect_v5_fused_kernel<E, true> against <E, false> on one v5-layout graph (levels G1, nc = 11, one pair of identical class rows
             per anchor): columns 0..4 bit-identical, conf = max_c fl32(cls_c obj), cls its first arg-max.

label -> cases                                                                                          worst |err| / bound on an MI355X: box rows, probability rows, sink conf
  detect_v8_kernel                   fp32: G1 x 4 widths, G2 x 2, stress; fed by 16-bit and split-precision
                                     convs (ADAS_NO_DETECT_FUSE=1, G1 x (64, 80, 80))                        0.150   0.713   -
  detect_v8_fused_kernel<Fp16>       G1 x 4 widths, G2 x 2, stress (box 0.079); sink: G1, G2 x 2 widths,
                                     with and without ties                                                   0.079   0.355   0.355
  detect_v8_fused_kernel<Bf16>       the same (stress: box 0.074)                                            0.074   0.362   0.362
  detect_v8_fused_x3_kernel          the same (stress: box 0.064)                                            0.064   0.401   0.401
  detect_v5_fused_kernel             sink against the rows of the same kernel without it, fp16 and bf16: bit-exact statements, no figure
The restatement's own ratios on these cases' operands (a CPU figure, printed per case, asserted <= 1): box rows up to 0.389 (the fp16
stress case), probability rows up to 0.820.  No sink case had an ambiguous anchor (0 of 492 / 1008 each); the tie groups lead on
424 .. 926 of 492 / 1008 anchors."""
import importlib

import numpy as np
import pytest

import conv_ref as CR
import detect_ref as D
import ops_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
load_pkg()
CE = importlib.import_module("adas_amd.coreEngine")
L = importlib.import_module("adas_amd._lib")
M = importlib.import_module("adas_amd.models")

NONE = R.ACT_NONE
GEOS = {"G1": ((9, 13), (5, 7), (3, 4)), "G2": ((16, 16), (8, 8), (4, 4))}
STRIDES = (8, 16, 32)
WIDTHS = ((64, 80, 80), (96, 40, 24), (32, 32, 8), (64, 64, 20))
BATCH = 3
IN_DETECT = "(fused into the Detect launch)"
FUSED_LABEL = {"fp16": "detect_v8_fused_kernel", "bf16": "detect_v8_fused_kernel", "fp16x3": "detect_v8_fused_x3_kernel"}
TIES = {80: ((3, 19, 40), (14, 17)), 24: ((3, 19), (14, 17))}
TIE_BIAS = 3.0
V5_NC, V5_PAIR = 11, (2, 7)
V5_ANCHORS = np.arange(10, 28, dtype=np.float32) * 3.0      # 3 levels x 3 anchors x (w, h): any 18 positive values


def head_graph(ws, geo, cb, cc, nc):
    """The v8-layout head of the module docstring on the level sizes `geo`."""
    (H, W) = geo[0]
    g = M.Graph("detunit", 3, H, W, ws)
    x, c3 = g.input()
    feats = [g.conv(x, 32, 1, 1, "expand", act=NONE, true_cin=c3)]
    feats.append(g.conv(feats[0], 32, 3, 2, "p4"))
    feats.append(g.conv(feats[1], 32, 3, 2, "p5"))
    assert tuple((f.h, f.w) for f in feats) == tuple(geo)
    ins = []
    for i, f in enumerate(feats):
        hb, hc = g.conv(f, cb, 1, 1, "hb%d" % i), g.conv(f, cc, 1, 1, "hc%d" % i)
        ins += [g.conv(hb, 64, 1, 1, "box%d" % i, act=NONE, f32_out=True), g.conv(hc, nc, 1, 1, "cls%d" % i, act=NONE, f32_out=True)]
    A = sum(f.h * f.w for f in feats)
    head = g.buf(1, 1, (4 + nc) * A, f32=True)
    g._op(M.OP_DETECT_V8, ins, head, params=[nc, A] + list(STRIDES), name="decode")
    g.output(head, 0, [1, 4 + nc, A], "output0")
    return g


def v5_graph(ws, geo, nc):
    """A v5-layout head: per level ONE 1x1 float32 conv to 3 (nc + 5) logits on the 32-channel feature map, then OP_DETECT_V5."""
    (H, W) = geo[0]
    g = M.Graph("det5unit", 3, H, W, ws)
    x, c3 = g.input()
    feats = [g.conv(x, 32, 1, 1, "expand", act=NONE, true_cin=c3)]
    feats.append(g.conv(feats[0], 32, 3, 2, "p4"))
    feats.append(g.conv(feats[1], 32, 3, 2, "p5"))
    ins = [g.conv(f, 3 * (nc + 5), 1, 1, "det%d" % i, act=NONE, f32_out=True) for i, f in enumerate(feats)]
    A = 3 * sum(f.h * f.w for f in feats)
    head = g.buf(1, 1, A * (nc + 5), f32=True)
    g._op(M.OP_DETECT_V5, ins, head, params=[nc, A] + list(STRIDES), name="decode")
    g.ops[-1]["w"] = g._blob(V5_ANCHORS)
    g.output(head, 0, [1, A, nc + 5], "output0")
    return g


def with_weights(build, override):
    """The graph on SynthWeights, or on a DictWeights copy of them with override(store) applied.  Returns (graph, the weights by name)."""
    ws = M.SynthWeights(17, gain=1.0)
    g = build(ws)
    if override is None:
        return g, ws.store
    d = {k: v.copy() for k, v in ws.store.items()}
    override(d)
    return build(M.DictWeights(d)), d


def stress_weights(d):
    for i in range(3):
        d["box%d.weight" % i] = (d["box%d.weight" % i] * 40.0).astype(np.float32)
        d["box%d.bias" % i] = np.linspace(-60, 60, 64).astype(np.float32)


def tie_weights(nc):
    def f(d):
        for i in range(3):
            w, b = d["cls%d.weight" % i], d["cls%d.bias" % i]
            for grp in TIES[nc]:
                for c in grp:
                    w[c], b[c] = w[grp[0]], TIE_BIAS
    return f


def v5_tie_weights(d):
    no = V5_NC + 5
    for i in range(3):
        w, b = d["det%d.weight" % i], d["det%d.bias" % i]
        for a in range(3):
            r0, r1 = a * no + 5 + V5_PAIR[0], a * no + 5 + V5_PAIR[1]
            w[r1], b[r0], b[r1] = w[r0], TIE_BIAS, TIE_BIAS


# ---- the cases: (id, geometry, (cb, cc, nc), precision, fused, stress);  test_detect_ref_cpu.py plans every one of them
def _cases():
    out = []
    for prec in ("fp32", "fp16", "bf16", "fp16x3"):
        for geo, widths in (("G1", WIDTHS), ("G2", WIDTHS[:2])):
            for wd in widths:
                out.append(("%s-%d.%d.%d-%s" % ((geo,) + wd + (prec,)), geo, wd, prec, prec != "fp32", False))
        out.append(("G1-stress-%s" % prec, "G1", WIDTHS[0], prec, prec != "fp32", True))
    for prec in ("fp16", "fp16x3"):
        out.append(("G1-64.80.80-%s-unfused" % prec, "G1", WIDTHS[0], prec, False, False))
    return out


CASES = _cases()
SINK_CASES = [("%s-%d.%d.%d-%s%s" % ((geo,) + wd + (prec, "-ties" if tie else "")), geo, wd, prec, tie)
              for geo in ("G1", "G2") for wd in WIDTHS[:2] for prec in ("fp16", "bf16", "fp16x3") for tie in (False, True)]
NOT_FUSABLE = ("G1", (64, 64, 22))      # planned on the CPU only: a float32 logits tensor whose width is no multiple of 4 is not conv_pw's, so nothing fuses


def case_graph(geo, wd, stress=False, tie=False):
    cb, cc, nc = wd
    over = stress_weights if stress else tie_weights(nc) if tie else None
    return with_weights(lambda ws: head_graph(ws, GEOS[geo], cb, cc, nc), over)


def frames(hw, seed=5):
    return np.random.default_rng(seed).uniform(-1, 1, (BATCH, 3) + tuple(hw)).astype(np.float32)


def expected_labels(fused, prec):
    lab = {"decode": FUSED_LABEL[prec] if fused else "detect_v8_kernel"}
    if fused:
        lab.update({"%s%d" % (n, i): IN_DETECT for n in ("box", "cls") for i in range(3)})
    return lab


def open_engine(tmp_path, g, prec, labels):
    path = str(tmp_path / "detunit.hipm")
    g.save(path)
    e = CE.HipEngine(path, prec, BATCH)
    try:
        for name, want in labels.items():
            got = e.layer_kernel(e.layer_index(name), BATCH)
            assert got == want, "%s resolves to %s, the case is written for %s" % (name, got, want)
        if "box0" in labels or labels["decode"] == "detect_v8_kernel":
            others = [e.layer_kernel(e.layer_index("%s%d" % (n, i)), BATCH) for n in ("box", "cls") for i in range(3)]
            assert all((k == IN_DETECT) == ("box0" in labels) for k in others), others
    except BaseException:
        e.close()
        raise
    return e


def reference(e, store, wd, prec, fused):
    """(want, bound, info) of the head from the operands the device fed the kernel; info carries the float64 logits."""
    info = {}
    if fused:
        hb, hc = [e.fetch_activation("hb%d" % i, BATCH) for i in range(3)], [e.fetch_activation("hc%d" % i, BATCH) for i in range(3)]
        for a in hb + hc:
            assert (a > 0).mean() > 0.1 and (a < 0).mean() > 0.1 and np.abs(a).max() < 1e3, "signed hidden maps"
        sw = lambda n: CR.weights_as_stored(store[n + ".weight"], prec)
        want, bound = D.v8_head_ref(hb, hc, [sw("box%d" % i) for i in range(3)], [store["box%d.bias" % i] for i in range(3)],
                                    [sw("cls%d" % i) for i in range(3)], [store["cls%d.bias" % i] for i in range(3)], STRIDES, prec, info=info)
    else:
        zb, zc = [e.fetch_activation("box%d" % i, BATCH) for i in range(3)], [e.fetch_activation("cls%d" % i, BATCH) for i in range(3)]
        want, bound = D.v8_logits_ref(zb, zc, STRIDES, "exact")
        flat = lambda a: a.reshape(a.shape[0], a.shape[1], -1)
        info.update(zb=[flat(z) for z in zb], zc=[flat(z) for z in zc], form="exact", max_box_logit=max(float(np.abs(z).max()) for z in zb),
                    max_cls_logit=max(float(np.abs(z).max()) for z in zc), max_dz=0.0)
    return want, bound, info


def judge(cid, label, geo, got, want, bound, info):
    """Prints the case's figures, then asserts: the float32 restatement inside the bound, every element of the head inside its bound."""
    yb, yp = D.decode_yardstick(info["zb"], info["zc"], GEOS[geo], STRIDES, info["form"])
    ok, rb, rp = D.check(got, want, bound)
    print("%s %s (%s form): worst |err| / bound box %.3f prob %.3f   yardstick box %.3f prob %.3f   max |box logit| %.1f |cls logit| %.1f  max dz %.2e  median bound box %.2e px prob %.2e"
          % (cid, label, info["form"], rb, rp, yb, yp, info["max_box_logit"], info["max_cls_logit"], info["max_dz"], float(np.median(bound[:, :4])), float(np.median(bound[:, 4:]))))
    assert yb <= 1.0 and yp <= 1.0, (yb, yp)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(~ok)
    assert ok.all(), (int((~ok).sum()), "frame, row, anchor:", bad[:8].tolist(), "rows", sorted(set(bad[:, 1].tolist()))[:12], "anchors", sorted(set(bad[:, 2].tolist()))[:12],
                      got[~ok][:4], want[~ok][:4], bound[~ok][:4])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_detect_head(tmp_path, monkeypatch, case):
    cid, geo, wd, prec, fused, stress = case
    if prec != "fp32" and not fused:
        monkeypatch.setenv("ADAS_NO_DETECT_FUSE", "1")
    g, store = case_graph(geo, wd, stress=stress)
    labels = expected_labels(fused, prec)
    e = open_engine(tmp_path, g, prec, labels)
    try:
        got = np.array(e.engine_inference(frames(GEOS[geo][0]))[0], copy=True)
        want, bound, info = reference(e, store, wd, prec, fused)
    finally:
        e.close()
    if stress:
        assert info["max_box_logit"] >= 100.0, info["max_box_logit"]
        assert np.isfinite(got).all()
    judge(cid, labels["decode"], geo, got, want, bound, info)


def run_with_sink(e, xin, n_rows):
    """The same frames with the sink set: (head, conf, cls, guard ok) -- conf / cls of n_rows entries in front of 64 guard entries."""
    conf, cls = L.DeviceBuffer.from_array(np.full(n_rows + 64, -7.0, np.float32)), L.DeviceBuffer.from_array(np.full(n_rows + 64, -7, np.int32))
    try:
        L.check(L.lib().adas_engine_set_detect_sink(e.handle, conf.ptr, cls.ptr))
        try:
            head = np.array(e.engine_inference(xin)[0], copy=True)
        finally:
            L.check(L.lib().adas_engine_set_detect_sink(e.handle, None, None))
        c, k = conf.download((n_rows + 64,), np.float32), cls.download((n_rows + 64,), np.int32)
    finally:
        conf.free()
        cls.free()
    return head, c[:n_rows], k[:n_rows], bool((c[n_rows:] == -7.0).all() and (k[n_rows:] == -7).all())


@pytest.mark.parametrize("case", SINK_CASES, ids=[c[0] for c in SINK_CASES])
def test_detect_sink(tmp_path, case):
    cid, geo, wd, prec, tie = case
    nc = wd[2]
    g, store = case_graph(geo, wd, tie=tie)
    labels = expected_labels(True, prec)
    xin = frames(GEOS[geo][0])
    e = open_engine(tmp_path, g, prec, labels)
    try:
        rows = np.array(e.engine_inference(xin)[0], copy=True)
        want, bound, info = reference(e, store, wd, prec, True)
        A = rows.shape[2]
        head, conf, cls, guards = run_with_sink(e, xin, BATCH * A)
    finally:
        e.close()
    judge(cid, labels["decode"], geo, rows, want, bound, info)
    conf, cls = conf.reshape(BATCH, A), cls.reshape(BATCH, A)
    # 1. every entry written, the guard entries untouched
    assert guards, "the sink wrote past its [batch][anchors] entries"
    assert (conf > 0).all() and (conf < 1).all() and (cls >= 0).all() and (cls < nc).all(), "an entry of the sink was not written"
    # 2. the box rows do not depend on the sink
    assert np.array_equal(head[:, :4].view(np.uint32), rows[:, :4].view(np.uint32))
    # 3. the same values and the first-maximum rule as the class rows of the run without the sink
    first = np.argmax(rows[:, 4:], 1)
    assert D.sink_matches_rows(conf, cls, rows[:, 4:]), ("conf differs on", int((conf != rows[:, 4:].max(1)).sum()), "cls differs at (frame, anchor)", np.argwhere(cls != first)[:8].tolist(),
                                                        cls[cls != first][:8], first[cls != first][:8])
    # 4. on its own against float64
    best, adm, amb = D.sink_ref(want[:, 4:], bound[:, 4:])
    lo, hi = (want[:, 4:] - bound[:, 4:]).max(1), (want[:, 4:] + bound[:, 4:]).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = float(np.max(np.where(conf == best, 0.0, np.abs(conf - best) / np.maximum(hi - best, best - lo))))
    print("%s sink: worst |conf - best| / bound %.3f   ambiguous anchors %d of %d" % (cid, r, int(amb.sum()), amb.size))
    assert ((conf >= lo) & (conf <= hi)).all()
    assert np.take_along_axis(adm, cls[:, None, :].astype(np.int64), 1).all(), "a class outside the admissible set"
    if tie:
        w, b = want[:, 4:], bound[:, 4:]
        groups = TIES[nc]
        member = np.zeros(nc, bool)
        member[[c for grp in groups for c in grp]] = True
        rest_hi = (w + b)[:, ~member].max(1)
        leads = []
        for gi, grp in enumerate(groups):
            other = groups[1 - gi][0]
            leads.append((w[:, grp[0]] - b[:, grp[0]] > rest_hi) & (w[:, grp[0]] - b[:, grp[0]] > w[:, other] + b[:, other]))
        n_lead = int(leads[0].sum() + leads[1].sum())
        print("%s ties: group %s leads on %d anchors, group %s on %d, of %d" % (cid, groups[0], int(leads[0].sum()), groups[1], int(leads[1].sum()), conf.size))
        assert leads[0].sum() > 0 and leads[1].sum() > 0 and n_lead > conf.size // 2
        for lead, grp in zip(leads, groups):
            assert (cls[lead] == grp[0]).all(), (grp, np.unique(cls[lead]).tolist())


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_detect_v5_sink(tmp_path, prec):
    """detect_v5_fused_kernel<E, true> against <E, false>: the sink takes max_c fl32(cls_c * obj) and its first arg-max from the same decoded row."""
    nc, no = V5_NC, V5_NC + 5
    g, _ = with_weights(lambda ws: v5_graph(ws, GEOS["G1"], nc), v5_tie_weights)
    labels = {"decode": "detect_v5_fused_kernel"}
    labels.update({"det%d" % i: IN_DETECT for i in range(3)})
    xin = frames(GEOS["G1"][0])
    e = open_engine(tmp_path, g, prec, labels)
    try:
        rows = np.array(e.engine_inference(xin)[0], copy=True)
        A = rows.shape[1]
        head, conf, cls, guards = run_with_sink(e, xin, BATCH * A)
    finally:
        e.close()
    assert rows.shape == (BATCH, 3 * sum(h * w for h, w in GEOS["G1"]), no) and np.isfinite(rows).all()
    assert guards, "the sink wrote past its [batch][rows] entries"
    conf, cls = conf.reshape(BATCH, A), cls.reshape(BATCH, A)
    assert (conf > 0).all() and (conf < 1).all() and (cls >= 0).all() and (cls < nc).all(), "an entry of the sink was not written"
    assert np.array_equal(head[..., :5].view(np.uint32), rows[..., :5].view(np.uint32))
    prod = (rows[..., 5:] * rows[..., 4:5]).astype(np.float32)
    assert prod.dtype == np.float32
    first = np.argmax(prod, -1)
    tied = prod[..., V5_PAIR[0]] == prod[..., V5_PAIR[1]]
    print("v5 sink %s: the pair %s ties on %d of %d rows and leads on %d" % (prec, V5_PAIR, int(tied.sum()), tied.size, int((first == V5_PAIR[0]).sum())))
    assert tied.all() and (first == V5_PAIR[0]).mean() > 0.5 and not (first == V5_PAIR[1]).any()
    assert np.array_equal(conf.view(np.uint32), prod.max(-1).view(np.uint32)), int((conf != prod.max(-1)).sum())
    assert np.array_equal(cls, first), (np.argwhere(cls != first)[:8].tolist(), cls[cls != first][:8], first[cls != first][:8])
