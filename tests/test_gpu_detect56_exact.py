"""GPU: the v5-layout and v6 Detect decode kernels, every element of the (B, A, nc + 5) head against float64 (tests/detect56_ref.py on top
of tests/detect_ref.py and tests/conv_ref.py; tests/test_detect56_ref_cpu.py judges that checker first and plans every graph of this file
on the CPU).

Pattern: input (signed uniform(-1, 1) frames, all distinct, batch 3) -> 1x1 "expand" with no activation = P3 (cin channels) -> 3x3 s2 SiLU
= P4 -> 3x3 s2 SiLU = P5, strides 8 / 16 / 32.  v5 layout: per level ONE 1x1 float32 conv "det<i>" to 3 (nc + 5) logits, OP_DETECT_V5 with
18 distinct anchors.  v6: per level 1x1 float32 convs "reg<i>" (4, or 68 with DFL) and "cls<i>" (nc), OP_DETECT_V6.  Operands of a
reference: the fetched float32 logits (detect_v5_kernel, detect_v6_kernel, detect_v6_dfl_kernel); the fetched 16-bit feature maps with the
weights as stored and the float32 bias (detect_v5_fused_kernel).  Every case asserts the decode's label (and "(fused into the Detect
launch)" on the three convs of a fused head), that the float32 restatement sits inside the bound on the case's own operands, and that
every element of the head is inside its bound; v6's objectness is compared with 1.0 for equality.

Geometries   G1  9x13 / 5x7 / 3x4 = 117 / 35 / 12 cells.  v6 (A = 164): both level boundaries inside a 32-row block, last block 4 rows.
                 v5 fused: one 128-cell block per anchor; waves with 21, 3 and 0 live rows.
             G2  16x16 / 8x8 / 4x4 = 256 / 64 / 16: boundaries on block boundaries.  v5 fused: exactly two blocks per anchor on level 0.
             G3  13x11 / 7x6 / 4x3 = 143 / 42 / 12.  v5 fused: a second block with 15 live rows in wave 0 and three idle waves.
v5 fused     (nc, cin) = (11, 32) no = 16, one full tile, one K step;  (3, 96) no = 8, half a tile, three K steps;  (28, 288) no = 33, one
             live row in tile 3, nine K steps: a full LDS chunk plus kc = 1;  (80, 288) no = 85, six tiles, the last with 5 live rows, a
             store loop of 6 passes;  (91, 512) no = 96, all tiles full, two full chunks.  Each on G3; (11, 32) and (80, 288) on G1, G2 too.
             slice: P3 is channels 8 .. 8 + cin of a wider buffer between guard channels of 1024.0 (x_coff = 8, x_cs = cin + 16).
             stress: logit weights x 40, bias linspace(-60, 60): logits past +-89 (asserted on the float64 logits), where __expf overflows
             resp. flushes; the head is finite.
             sink: (80, 288) on G3, rows held to float64, then columns 0..4 bit-identical and conf / cls the float32 maximum and first
             arg-max of the same run's rows (tests/test_gpu_detect_exact.py::test_detect_v5_sink's statements, one tied pair per row).
v5 plain     fp32 and fp16x3 (nothing fuses): G1, G3 x nc 11, 80.  fp16 / bf16 convs in front: nc = 92 (no = 97 > 96 cannot fuse).
             loop: 40x36 / 20x18 / 10x9, nc = 91, fp32: A no = 5670 x 96 = 544 320 > 2048 x 256, the grid-stride loop's second trip.
v6, v6 DFL   fp32: G1, G2 x nc 80, 20, 3 (no = 8: 256 elements, exactly one pass), 1;  fp16, bf16, fp16x3: G1 x 80 (the logits stay
             float32).  wide: reg / cls are the leading channels of float32 buffers with four trailing sentinel channels of 1024.0
             (reg_cs = 8 resp. 72, cls_cs = nc + 4 = 24).  DFL also: stress (reg weights x 40, a bias ramp over the bins, max |z| >= 100
             asserted on the fetched logits), argmax (bin 0 leads on side 0, bin 16 on side 2: asserted), equal (weights 0, one bias:
             every distance is 8 within the softmax bound).

label -> cases                                                                                  worst |err| / bound on an MI355X: box, other columns
  detect_v5_kernel                 fp32, fp16x3: G1, G3 x nc 11, 80; fp16, bf16: nc 92; loop                 0.623   0.730
  detect_v5_fused_kernel<Fp16>     5 widths on G3, 2 on G1, G2; slice; stress; sink                          0.423   0.907
  detect_v5_fused_kernel<Bf16>     the same                                                                  0.443   0.993
  detect_v6_kernel                 fp32: G1, G2 x 4 widths, wide; 3 more precisions on G1                    0.949   0.724
  detect_v6_dfl_kernel             the same; stress, argmax, equal                                           0.140   0.716
Reported, fed back into nothing.  The fused kernel's 0.907 / 0.993 are the stress case's (a saturated column, where the restatement on the
same operands gives the same figure); detect_v6_kernel's 0.949 is the restatement's own on those operands: IEEE roundings alone.  The
restatement's ratios on the cases' fetched operands (a CPU figure, asserted <= 1): up to 0.713 / 0.993 (v5 fused), 0.687 / 0.823 (v5),
0.949 / 0.810 (v6), 0.119 / 0.820 (DFL).  The sink's pair ties on all 1773 rows and leads on 1155.  62 tests, 3.3 s
(tests/test_gpu_detect_exact.py in the same session: 56 tests, 2.7 s)."""
import importlib

import numpy as np
import pytest

import conv_ref as CR
import detect56_ref as R6
import ops_ref as R
import test_gpu_detect_exact as GD
from conftest import load_pkg

pytestmark = pytest.mark.gpu
load_pkg()
CE = importlib.import_module("adas_amd.coreEngine")
M = importlib.import_module("adas_amd.models")

NONE = R.ACT_NONE
GEOS = dict(GD.GEOS, G3=((13, 11), (7, 6), (4, 3)), LOOP=((40, 36), (20, 18), (10, 9)))
STRIDES = GD.STRIDES
BATCH = GD.BATCH
IN_DETECT = GD.IN_DETECT
ANCHORS = GD.V5_ANCHORS
GUARD = 1024.0                                    # exact in every storage type
FUSED_WIDTHS = ((11, 32), (3, 96), (28, 288), (80, 288), (91, 512))
SINK_WIDTH, SINK_GEO, SINK_PAIR = (80, 288), "G3", GD.V5_PAIR
V6_NCS = (80, 20, 3, 1)
WIDE_NC = 20
OVERFLOW_Z = 89.0                                 # __expf(-z) = exp2(-z log2 e) leaves float32 at |z| = 128 ln 2 = 88.7
PRECS = ("fp32", "fp16", "bf16", "fp16x3")
WORST = {}                                        # label -> [box, other]: printed, asserted nowhere


def _feats(g, x, c3, cin, sliced):
    if sliced:
        cat = g.buf(x.h, x.w, cin + 16)
        for nm, off in (("guard_lo", 0), ("guard_hi", 8 + cin)):
            g.conv(x, 8, 1, 1, nm, act=NONE, true_cin=c3, out=cat.slice(off, 8), weight=np.zeros((8, c3, 1, 1), np.float32), bias_fill=GUARD)
        feats = [g.conv(x, cin, 1, 1, "expand", act=NONE, true_cin=c3, out=cat.slice(8, cin))]
    else:
        feats = [g.conv(x, cin, 1, 1, "expand", act=NONE, true_cin=c3)]
    feats.append(g.conv(feats[0], cin, 3, 2, "p4"))
    feats.append(g.conv(feats[1], cin, 3, 2, "p5"))
    return feats


def v5_graph(ws, geo, nc, cin=32, sliced=False):
    """The v5-layout head of the module docstring on the level sizes `geo`."""
    (H, W) = geo[0]
    g = M.Graph("det5unit", 3, H, W, ws)
    x, c3 = g.input()
    feats = _feats(g, x, c3, cin, sliced)
    assert tuple((f.h, f.w) for f in feats) == tuple(geo)
    ins = [g.conv(f, 3 * (nc + 5), 1, 1, "det%d" % i, act=NONE, f32_out=True) for i, f in enumerate(feats)]
    A = 3 * sum(f.h * f.w for f in feats)
    head = g.buf(1, 1, A * (nc + 5), f32=True)
    g._op(M.OP_DETECT_V5, ins, head, params=[nc, A] + list(STRIDES), name="decode")
    g.ops[-1]["w"] = g._blob(ANCHORS)
    g.output(head, 0, [1, A, nc + 5], "output0")
    return g


def v6_graph(ws, geo, nc, dfl, wide=False):
    """The v6 head of the module docstring; wide: reg<i> / cls<i> lead float32 buffers with four trailing sentinel channels."""
    (H, W) = geo[0]
    g = M.Graph("det6unit", 3, H, W, ws)
    x, c3 = g.input()
    feats = _feats(g, x, c3, 32, False)
    assert tuple((f.h, f.w) for f in feats) == tuple(geo)
    nreg = 4 * R6.DFL_BINS if dfl else 4
    ins = []
    for i, f in enumerate(feats):
        if wide:
            rb, cb = g.buf(f.h, f.w, nreg + 4, f32=True), g.buf(f.h, f.w, nc + 4, f32=True)
            for nm, b_, off in (("regs%d" % i, rb, nreg), ("clss%d" % i, cb, nc)):
                g.conv(f, 4, 1, 1, nm, act=NONE, out=b_.slice(off, 4), weight=np.zeros((4, f.c, 1, 1), np.float32), bias_fill=GUARD)
            ins += [g.conv(f, nreg, 1, 1, "reg%d" % i, act=NONE, out=rb.slice(0, nreg)), g.conv(f, nc, 1, 1, "cls%d" % i, act=NONE, out=cb.slice(0, nc))]
        else:
            ins += [g.conv(f, nreg, 1, 1, "reg%d" % i, act=NONE, f32_out=True), g.conv(f, nc, 1, 1, "cls%d" % i, act=NONE, f32_out=True)]
    A = sum(f.h * f.w for f in feats)
    head = g.buf(1, 1, A * (nc + 5), f32=True)
    g._op(M.OP_DETECT_V6, ins, head, params=[nc, A] + list(STRIDES) + ([M.V6_REG_MAX] if dfl else []), name="decode")
    g.output(head, 0, [1, A, nc + 5], "output0")
    return g


# ---- weight overrides (on a copy of the seeded weights)
def v5_stress(d):
    for i in range(3):
        d["det%d.weight" % i] = (d["det%d.weight" % i] * 40.0).astype(np.float32)
        d["det%d.bias" % i] = np.linspace(-60, 60, d["det%d.bias" % i].size).astype(np.float32)


def v5_tie(nc):
    def f(d):
        no = nc + 5
        for i in range(3):
            w, b = d["det%d.weight" % i], d["det%d.bias" % i]
            for a in range(3):
                r0, r1 = a * no + 5 + SINK_PAIR[0], a * no + 5 + SINK_PAIR[1]
                w[r1], b[r0], b[r1] = w[r0], GD.TIE_BIAS, GD.TIE_BIAS
    return f


def dfl_stress(d):
    for i in range(3):
        d["reg%d.weight" % i] = (d["reg%d.weight" % i] * 40.0).astype(np.float32)
        d["reg%d.bias" % i] = np.tile(np.linspace(-60, 60, R6.DFL_BINS), 4).astype(np.float32)


def dfl_argmax(d):
    for i in range(3):
        b = d["reg%d.bias" % i]
        b[0], b[2 * R6.DFL_BINS + 16] = 30.0, 30.0


def dfl_equal(d):
    for i in range(3):
        d["reg%d.weight" % i][:] = 0.0
        d["reg%d.bias" % i][:] = 1.5


V5_OVER = {"stress": v5_stress, "tie": v5_tie(SINK_WIDTH[0])}
DFL_OVER = {"stress": dfl_stress, "argmax": dfl_argmax, "equal": dfl_equal}


# ---- the cases; tests/test_detect56_ref_cpu.py plans every one of them
def _fused_cases():
    out = []
    for prec in ("fp16", "bf16"):
        for geo, widths in (("G3", FUSED_WIDTHS), ("G1", (FUSED_WIDTHS[0], FUSED_WIDTHS[3])), ("G2", (FUSED_WIDTHS[0], FUSED_WIDTHS[3]))):
            out += [("%s-%d.%d-%s" % (geo, nc, cin, prec), geo, nc, cin, prec, None) for nc, cin in widths]
        out.append(("G3-28.288-%s-slice" % prec, "G3", 28, 288, prec, "slice"))
        out.append(("G1-11.32-%s-stress" % prec, "G1", 11, 32, prec, "stress"))
    return out


def _plain_cases():
    out = [("%s-%d-%s" % (geo, nc, prec), geo, nc, prec) for prec in ("fp32", "fp16x3") for geo in ("G1", "G3") for nc in (11, 80)]
    out += [("G1-92-%s" % prec, "G1", 92, prec) for prec in ("fp16", "bf16")]
    return out + [("LOOP-91-fp32", "LOOP", 91, "fp32")]


def _v6_cases():
    out = []
    for dfl in (False, True):
        tag = "dfl-" if dfl else ""
        out += [("%s%s-%d-fp32" % (tag, geo, nc), dfl, geo, nc, "fp32", None) for geo in ("G1", "G2") for nc in V6_NCS]
        out.append(("%sG1-%d-fp32-wide" % (tag, WIDE_NC), dfl, "G1", WIDE_NC, "fp32", "wide"))
        out += [("%sG1-80-%s" % (tag, prec), dfl, "G1", 80, prec, None) for prec in PRECS[1:]]
    return out + [("dfl-G1-80-fp32-%s" % k, True, "G1", 80, "fp32", k) for k in DFL_OVER]


FUSED_CASES, PLAIN_CASES, V6_CASES = _fused_cases(), _plain_cases(), _v6_cases()


def fused_graph(geo, nc, cin, kind=None):
    return GD.with_weights(lambda ws: v5_graph(ws, GEOS[geo], nc, cin, sliced=kind == "slice"), V5_OVER.get(kind))


def v6_case_graph(dfl, geo, nc, kind=None):
    return GD.with_weights(lambda ws: v6_graph(ws, GEOS[geo], nc, dfl, wide=kind == "wide"), DFL_OVER.get(kind))


def v5_labels(fused):
    lab = {"decode": "detect_v5_fused_kernel" if fused else "detect_v5_kernel"}
    if fused:
        lab.update({"det%d" % i: IN_DETECT for i in range(3)})
    return lab


def open_engine(tmp_path, g, prec, labels, not_in_detect=()):
    path = str(tmp_path / "det56unit.hipm")
    g.save(path)
    e = CE.HipEngine(path, prec, BATCH)
    try:
        for name, want in labels.items():
            got = e.layer_kernel(e.layer_index(name), BATCH)
            assert got == want, "%s resolves to %s, the case is written for %s" % (name, got, want)
        for name in not_in_detect:
            assert e.layer_kernel(e.layer_index(name), BATCH) != IN_DETECT, name
    except BaseException:
        e.close()
        raise
    return e


def judge(cid, label, got, want, bound, yard, extra=""):
    """Prints the case's figures, then asserts: the float32 restatement inside the bound, every element of the head inside its bound."""
    ok, rb, rp = R6.check(got, want, bound)
    w = WORST.setdefault(label, [0.0, 0.0])
    w[0], w[1] = max(w[0], rb), max(w[1], rp)
    print("%s %s: worst |err| / bound box %.3f other %.3f   yardstick box %.3f other %.3f   median bound box %.2e px other %.2e   so far for this label: box %.3f other %.3f  %s"
          % (cid, label, rb, rp, yard[0], yard[1], float(np.median(bound[..., :4])), float(np.median(bound[..., 5:])), w[0], w[1], extra))
    assert yard[0] <= 1.0 and yard[1] <= 1.0, yard
    bad = np.argwhere(~ok)
    assert ok.all(), (int((~ok).sum()), "frame, row, column:", bad[:8].tolist(), "rows", sorted(set(bad[:, 1].tolist()))[:12], "columns", sorted(set(bad[:, 2].tolist()))[:12],
                      got[~ok][:4], want[~ok][:4], bound[~ok][:4])


def fused_reference(e, store, geo, prec):
    """(want, bound, info) of the fused head from the feature maps the device fed the kernel."""
    feats = [e.fetch_activation(n, BATCH) for n in ("expand", "p4", "p5")]
    for a in feats:
        assert (a > 0).mean() > 0.1 and (a < 0).mean() > 0.1 and np.abs(a).max() < 1e3, "signed feature maps"
    info = {}
    want, bound = R6.v5_head_ref(feats, [CR.weights_as_stored(store["det%d.weight" % i], prec) for i in range(3)], [store["det%d.bias" % i] for i in range(3)],
                                 GEOS[geo], STRIDES, ANCHORS, prec, info=info)
    return want, bound, info


def v5_yard(info, geo):
    return R6.v5_yardstick(info["z"], GEOS[geo], STRIDES, ANCHORS, info["form"])


@pytest.mark.parametrize("case", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_detect_v5_fused(tmp_path, case):
    cid, geo, nc, cin, prec, kind = case
    g, store = fused_graph(geo, nc, cin, kind)
    e = open_engine(tmp_path, g, prec, v5_labels(True))
    try:
        got = np.array(e.engine_inference(GD.frames(GEOS[geo][0]))[0], copy=True)
        want, bound, info = fused_reference(e, store, geo, prec)
        guards = [e.fetch_activation(n, BATCH) for n in ("guard_lo", "guard_hi")] if kind == "slice" else []
    finally:
        e.close()
    for a in guards:
        assert a.shape[1] == 8 and (a == GUARD).all(), "a guard channel was overwritten"
    if kind == "stress":
        assert info["min_z"] <= -OVERFLOW_Z and info["max_z"] >= OVERFLOW_Z, (info["min_z"], info["max_z"])
        assert np.isfinite(got).all()
    judge(cid, "detect_v5_fused_kernel<%s>" % prec, got, want, bound, v5_yard(info, geo), "logits %.1f .. %.1f  max dz %.2e" % (info["min_z"], info["max_z"], info["max_dz"]))


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_detect_v5_sink_wide(tmp_path, prec):
    """tests/test_gpu_detect_exact.py::test_detect_v5_sink's statements at no = 85, cin = 288 on G3, behind the float64 check of the rows."""
    nc, cin = SINK_WIDTH
    g, store = fused_graph(SINK_GEO, nc, cin, "tie")
    xin = GD.frames(GEOS[SINK_GEO][0])
    e = open_engine(tmp_path, g, prec, v5_labels(True))
    try:
        rows = np.array(e.engine_inference(xin)[0], copy=True)
        want, bound, info = fused_reference(e, store, SINK_GEO, prec)
        A = rows.shape[1]
        head, conf, cls, guards = GD.run_with_sink(e, xin, BATCH * A)
    finally:
        e.close()
    judge("sink-%s" % prec, "detect_v5_fused_kernel<%s>" % prec, rows, want, bound, v5_yard(info, SINK_GEO))
    assert rows.shape == (BATCH, 3 * sum(h * w for h, w in GEOS[SINK_GEO]), nc + 5)
    assert guards, "the sink wrote past its [batch][rows] entries"
    conf, cls = conf.reshape(BATCH, A), cls.reshape(BATCH, A)
    assert (conf > 0).all() and (conf < 1).all() and (cls >= 0).all() and (cls < nc).all(), "an entry of the sink was not written"
    assert np.array_equal(head[..., :5].view(np.uint32), rows[..., :5].view(np.uint32))
    prod = (rows[..., 5:] * rows[..., 4:5]).astype(np.float32)
    assert prod.dtype == np.float32
    first = np.argmax(prod, -1)
    tied = prod[..., SINK_PAIR[0]] == prod[..., SINK_PAIR[1]]
    print("v5 sink %s: the pair %s ties on %d of %d rows and leads on %d" % (prec, SINK_PAIR, int(tied.sum()), tied.size, int((first == SINK_PAIR[0]).sum())))
    assert tied.all() and (first == SINK_PAIR[0]).mean() > 0.5 and not (first == SINK_PAIR[1]).any()
    assert np.array_equal(conf.view(np.uint32), prod.max(-1).view(np.uint32)), int((conf != prod.max(-1)).sum())
    assert np.array_equal(cls, first), (np.argwhere(cls != first)[:8].tolist(), cls[cls != first][:8], first[cls != first][:8])


@pytest.mark.parametrize("case", PLAIN_CASES, ids=[c[0] for c in PLAIN_CASES])
def test_detect_v5_plain(tmp_path, case):
    cid, geo, nc, prec = case
    g, _ = GD.with_weights(lambda ws: v5_graph(ws, GEOS[geo], nc), None)
    e = open_engine(tmp_path, g, prec, v5_labels(False), not_in_detect=["det%d" % i for i in range(3)])
    try:
        got = np.array(e.engine_inference(GD.frames(GEOS[geo][0]))[0], copy=True)
        logits = [e.fetch_activation("det%d" % i, BATCH) for i in range(3)]
    finally:
        e.close()
    info = {}
    want, bound = R6.v5_logits_ref(logits, GEOS[geo], STRIDES, ANCHORS, info=info)
    if geo == "LOOP":
        assert want[0].size > 2048 * 256
    judge(cid, "detect_v5_kernel", got, want, bound, v5_yard(info, geo), "logits %.1f .. %.1f" % (info["min_z"], info["max_z"]))


@pytest.mark.parametrize("case", V6_CASES, ids=[c[0] for c in V6_CASES])
def test_detect_v6(tmp_path, case):
    cid, dfl, geo, nc, prec, kind = case
    g, _ = v6_case_graph(dfl, geo, nc, kind)
    label = "detect_v6_dfl_kernel" if dfl else "detect_v6_kernel"
    e = open_engine(tmp_path, g, prec, {"decode": label})
    try:
        got = np.array(e.engine_inference(GD.frames(GEOS[geo][0]))[0], copy=True)
        reg, cls = [e.fetch_activation("reg%d" % i, BATCH) for i in range(3)], [e.fetch_activation("cls%d" % i, BATCH) for i in range(3)]
        sent = [e.fetch_activation("%s%d" % (n, i), BATCH) for n in ("regs", "clss") for i in range(3)] if kind == "wide" else []
    finally:
        e.close()
    for a in sent:
        assert a.shape[1] == 4 and (a == GUARD).all(), "a sentinel channel was overwritten"
    sizes = GEOS[geo]
    assert [a.shape for a in reg] == [(BATCH, 68 if dfl else 4) + hw for hw in sizes] and [a.shape for a in cls] == [(BATCH, nc) + hw for hw in sizes]
    want, bound = R6.v6_ref(reg, cls, sizes, STRIDES, dfl)
    assert (got[..., 4] == 1.0).all(), "objectness is exactly 1.0f"
    zmax = max(float(np.abs(a).max()) for a in reg)
    if kind == "stress":
        assert zmax >= 100.0, zmax
        assert np.isfinite(got).all()
    if kind == "argmax":
        for a in reg:
            z = a.reshape(BATCH, 4, R6.DFL_BINS, -1)
            assert (z[:, 0].argmax(1) == 0).all() and (z[:, 2].argmax(1) == 16).all()
    if kind == "equal":
        st = np.concatenate([np.full(h * w, float(s)) for (h, w), s in zip(sizes, STRIDES)])
        assert np.abs(want[..., 2] - 16 * st).max() < 1e-9 and np.abs(want[..., 3] - 16 * st).max() < 1e-9, "every distance is 8"
    judge(cid, label, got, want, bound, R6.v6_yardstick(reg, cls, sizes, STRIDES, dfl), "max |reg| %.1f" % zmax)
