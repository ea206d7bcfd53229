"""CPU tests of tests/detect_ref.py, the per-element checker of tests/test_gpu_detect_exact.py, and of that file's graphs.  Before a kernel
is judged: the reference agrees with the oracle's v8 decode; the float32 restatements of the decode (both sigmoid forms, exp and
reciprocal results +-1 ulp) sit inside the bound, closely enough to the recorded ratios; the checker REJECTS each way a Detect kernel can
go wrong locally, in every geometry; the bound leaves next to no anchor without a definite best class; and every graph of the GPU file
plans onto the kernel its case names (include/adas_hip.h adas_debug_engine_plan: no device)."""
import numpy as np
import pytest
import torch

import conv_ref as CR
import detect_ref as D
import ops_ref as R
import test_gpu_detect_exact as GD
from oracle import nets
from test_engine_plan_cpu import BF16, CONV_DET5, CONV_PW, DET_SRC, F16, F32, KERNEL, SKIP, X3, env, idx, plan

M = GD.M
F = np.float32
PREC_ID = {"fp32": F32, "fp16": F16, "bf16": BF16, "fp16x3": X3}
GEO_WIDTHS = [(geo, wd) for geo, widths in (("G1", GD.WIDTHS), ("G2", GD.WIDTHS[:2])) for wd in widths]


def operands(geo, wd, prec, seed=0, stress=False, tie=False):
    """Synthetic operands of the fused head: hidden maps uniform(-1, 1) rounded to the storage type, weights N(0, 1 / cin) as stored."""
    cb, cc, nc = wd
    rng = np.random.default_rng(seed)
    hb = [R.storage_round(rng.uniform(-1, 1, (GD.BATCH, cb) + hw).astype(F), prec) for hw in GD.GEOS[geo]]
    hc = [R.storage_round(rng.uniform(-1, 1, (GD.BATCH, cc) + hw).astype(F), prec) for hw in GD.GEOS[geo]]
    wb = [(rng.standard_normal((64, cb, 1, 1)) / np.sqrt(cb)).astype(F) for _ in range(3)]
    wc = [(rng.standard_normal((nc, cc, 1, 1)) / np.sqrt(cc)).astype(F) for _ in range(3)]
    bb, bc = [(rng.standard_normal(64) * 0.05).astype(F) for _ in range(3)], [(rng.standard_normal(nc) * 0.05).astype(F) for _ in range(3)]
    if stress:
        wb, bb = [(w * 40).astype(F) for w in wb], [np.linspace(-60, 60, 64).astype(F) for _ in range(3)]
    if tie:
        for w, b in zip(wc, bc):
            for grp in GD.TIES[nc]:
                for c in grp:
                    w[c], b[c] = w[grp[0]], GD.TIE_BIAS
    st = lambda ws: [CR.weights_as_stored(w, prec) for w in ws]
    return hb, hc, st(wb), bb, st(wc), bc


def head(geo, wd, prec, **kw):
    """(want, bound, info, the float32 logits) of a synthetic case."""
    info = {}
    want, bound = D.v8_head_ref(*operands(geo, wd, prec, **kw), GD.STRIDES, prec, info=info)
    return want, bound, info, [z.astype(F) for z in info["zb"]], [z.astype(F) for z in info["zc"]]


# ------------------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("geo", ["G1", "G2"])
def test_reference_agrees_with_the_oracle(geo):
    """detect_ref's float64 decode against oracle/nets.py _v8_decode (torch float32) on the same float32 logits, with the strides the oracle
    derives from the map sizes (G1: 8, 14, 24 -- no powers of two).  What float32 explains: the exact-form bound at dz = 0, doubled --
    torch normalises every bin before it weights it (one more division per bin) and sums in its own order."""
    sizes, nc = GD.GEOS[geo], 24
    rng = np.random.default_rng(4)
    outs = [rng.normal(0, 2, (GD.BATCH, 64 + nc, h * w)).astype(F) for h, w in sizes]
    got = nets._v8_decode([torch.from_numpy(o) for o in outs], sizes, nc)
    strides = [sizes[0][0] * 8 // h for h, _ in sizes]
    want, bound = D.decode_ref([o[:, :64] for o in outs], [o[:, 64:] for o in outs], None, None, sizes, strides, "exact")
    ok, rb, rp = D.check(got, want, 2 * bound)
    print("oracle v8 decode vs float64 on %s (strides %s): worst |diff| / (2 x bound) box %.3f prob %.3f; max |diff| box %.2e px prob %.2e"
          % (geo, strides, rb, rp, np.abs(got - want)[:, :4].max(), np.abs(got - want)[:, 4:].max()))
    assert got.shape == want.shape == (GD.BATCH, 4 + nc, sum(h * w for h, w in sizes)) and ok.all()


def test_reference_is_the_expression_written_out():
    """One cell by hand: scalar Python on the stated formulas."""
    rng = np.random.default_rng(1)
    zb, zc = rng.normal(0, 3, (1, 64, 6)), rng.normal(0, 3, (1, 5, 6))
    want, bound = D.decode_ref([zb], [zc], None, None, [(2, 3)], [16], "fast")
    p = 4                                     # cell (y, x) = (1, 1)
    dist = [float((np.exp(zb[0, s * 16:s * 16 + 16, p]) * np.arange(16)).sum() / np.exp(zb[0, s * 16:s * 16 + 16, p]).sum()) for s in range(4)]
    x1, y1, x2, y2 = 1.5 - dist[0], 1.5 - dist[1], 1.5 + dist[2], 1.5 + dist[3]
    assert np.allclose(want[0, :4, p], [(x1 + x2) / 2 * 16, (y1 + y2) / 2 * 16, (x2 - x1) * 16, (y2 - y1) * 16], rtol=0, atol=1e-11)
    assert np.allclose(want[0, 4:, p], 1 / (1 + np.exp(-zc[0, :, p])), rtol=0, atol=1e-15) and (bound > 0).all()


# ------------------------------------------------------------------------------------------------------------------------- the restatements
def test_restatements_sit_inside_the_bound():
    """decode_f32 in both forms on every geometry and width and on the stress logits, from float32(logits) at the rounding's own dz: inside
    the bound, and the worst ratios are the ones detect_ref records (held to within 15 % below)."""
    worst = {f: [0.0, 0.0] for f in D.FORMS}
    for geo, wd, stress in [(g_, w_, False) for g_, w_ in GEO_WIDTHS] + [("G1", GD.WIDTHS[0], True)]:
        _, _, info, _, _ = head(geo, wd, "fp16", seed=3, stress=stress)
        if stress:
            assert info["max_box_logit"] >= 100
        for form in D.FORMS:
            for seed in range(3):
                rb, rp = D.decode_yardstick(info["zb"], info["zc"], GD.GEOS[geo], GD.STRIDES, form, seed)
                worst[form] = [max(worst[form][0], rb), max(worst[form][1], rp)]
    print("decode restatements, worst |f32 - f64| / bound: " + "  ".join("%s form box %.3f prob %.3f" % (f, worst[f][0], worst[f][1]) for f in D.FORMS))
    for f in D.FORMS:
        for got, rec in zip(worst[f], D.YARD[f]):
            assert 0.85 * rec <= got <= rec <= 1.0, (f, worst[f], D.YARD[f])


def test_restatement_covers_whole_fused_head():
    """With the float32 conv in front (torch float32 conv2d on the same operands) the restatement sits inside the fused head's bound."""
    for prec in ("fp16", "bf16", "fp16x3"):
        ops = operands("G1", GD.WIDTHS[1], prec, seed=5)
        want, bound = D.v8_head_ref(*ops, GD.STRIDES, prec)
        hb, hc, wb, bb, wc, bc = ops
        z32 = lambda x, w, b: (CR.acc_f32_torch(x, w, 1, 0) + b[None, :, None, None]).astype(F).reshape(x.shape[0], w.shape[0], -1)
        got = D.decode_f32([z32(hb[l], wb[l], bb[l]) for l in range(3)], [z32(hc[l], wc[l], bc[l]) for l in range(3)], GD.GEOS["G1"], GD.STRIDES, D.form_of(prec, True))
        ok, rb, rp = D.check(got, want, bound)
        print("float32 head %s: worst |f32 - f64| / bound box %.3f prob %.3f" % (prec, rb, rp))
        assert ok.all()


# ------------------------------------------------------------------------------------------------------------------------- wrong kernels
def _offsets(geo):
    hw = [h * w for h, w in GD.GEOS[geo]]
    return hw, [0, hw[0], hw[0] + hw[1]]


def _anchor_no_half(out, geo, **_):
    hw, off = _offsets(geo)
    for l in range(3):
        out[:, :2, off[l]:off[l] + hw[l]] -= F(0.5 * GD.STRIDES[l])
    return out


def _a_off_by_one(out, geo, **_):
    hw, off = _offsets(geo)
    blk = out[:, :, off[1]:off[1] + hw[1]].copy()
    out[:, :, off[1]] = 0
    out[:, :, off[1] + 1:off[1] + 1 + hw[1]] = blk
    return out


def _tail_unwritten(out, geo, **_):
    hw, off = _offsets(geo)
    l = [i for i in range(3) if hw[i] % 64][0]
    out[:, :, off[l] + hw[l] // 64 * 64:off[l] + hw[l]] = 0
    return out


def _tile_rotated(out, geo, **_):
    out[:, 4:] = np.roll(out[:, 4:], 16, 1)
    return out


def _classes_dropped(out, geo, nc, **_):
    out[:, 4 + 16 * (nc // 16):] = 0
    return out


def _half_ulp(which, prec):
    def f(zb, zc, geo):
        z = (zb if which == "box" else zc)[0]
        near = np.abs(z - 1.0)
        if which == "box":          # an outermost bin: |k - dist| is not small by accident
            near[:, [k for k in range(64) if k % 16 not in (0, 15)]] = np.inf
        i = np.unravel_index(np.argmin(near), z.shape)
        assert 0.8 < z[i] < 1.2
        z[i] += F(2.0 ** -11 if prec == "fp16" else 2.0 ** -8)        # half an ulp of the storage type in [1, 2)
        return zb, zc
    return f


def _sides_swapped(zb, zc, geo):
    for z in zb:
        z[:, 16:48] = np.concatenate([z[:, 32:48], z[:, 16:32]], 1)
    return zb, zc


# name -> (on the logits, inside the softmax, on the strides, on the output, the class counts for which it changes nothing)
WRONG = {
    "bins-weighted-k+1": (None, dict(bins=np.arange(1, 17)), None, None, ()),
    "anchor-without-0.5": (None, {}, None, _anchor_no_half, ()),
    "neighbours-stride": (None, {}, (8, 8, 32), None, ()),
    "a_off-of-level-1-off-by-one": (None, {}, None, _a_off_by_one, ()),
    "tail-block-unwritten": (None, {}, None, _tail_unwritten, ()),
    "class-tile-rotated": (None, {}, None, _tile_rotated, (8,)),
    "classes-past-the-full-tiles-dropped": (None, {}, None, _classes_dropped, (80,)),
    "sides-1-and-2-swapped": (_sides_swapped, {}, None, None, ()),
    "box-logit-half-ulp-fp16": (_half_ulp("box", "fp16"), {}, None, None, ()),
    "cls-logit-half-ulp-fp16": (_half_ulp("cls", "fp16"), {}, None, None, ()),
    "box-logit-half-ulp-bf16": (_half_ulp("box", "bf16"), {}, None, None, ()),
    "cls-logit-half-ulp-bf16": (_half_ulp("cls", "bf16"), {}, None, None, ()),
}


@pytest.mark.parametrize("geo", ["G1", "G2"])
@pytest.mark.parametrize("name", list(WRONG))
def test_wrong_kernels_are_rejected(name, geo):
    """Each mistake, on every width of the geometry, in the form of the precision it is stated for: the unmutated restatement passes, the
    mutated one fails, and a mutation that changes nothing (a tile rotation of 8 classes, no class past five full tiles of 80) occurs only
    where it is expected and never for every width of a geometry."""
    on_logits, inside, strides, on_output, vacuous_nc = WRONG[name]
    prec = "bf16" if name.endswith("bf16") else "fp16"
    real = 0
    for g_, wd in GEO_WIDTHS:
        if g_ != geo:
            continue
        want, bound, info, zb, zc = head(geo, wd, prec, seed=2)
        form = info["form"]
        good = D.decode_f32(zb, zc, GD.GEOS[geo], GD.STRIDES, form)
        assert D.check(good, want, bound)[0].all()
        mb, mc = on_logits([z.copy() for z in zb], [z.copy() for z in zc], geo) if on_logits else (zb, zc)
        bad = D.decode_f32(mb, mc, GD.GEOS[geo], strides or GD.STRIDES, form, **inside)
        if on_output:
            bad = on_output(bad.copy(), geo, nc=wd[2])
        if np.array_equal(bad, good):
            assert wd[2] in vacuous_nc, (name, wd)
            continue
        real += 1
        ok, rb, rp = D.check(bad, want, bound)
        assert not ok.all(), (name, geo, wd, rb, rp)
        if "half-ulp" in name:      # one storage rounding of the head's input is several bounds away, not just outside
            print("%s %s %s: |err| / bound box %.1f prob %.1f" % (name, geo, wd, rb, rp))
            assert max(rb, rp) > 4, (name, geo, wd, rb, rp)
    assert real >= 1


@pytest.mark.parametrize("form", D.FORMS)
def test_softmax_without_the_maximum_is_rejected_on_the_stress_case(form):
    want, bound, info, zb, zc = head("G1", GD.WIDTHS[0], "fp16", seed=2, stress=True)
    assert info["max_box_logit"] >= 100 and info["max_cls_logit"] <= D.SIG_Z_MAX
    assert D.check(D.decode_f32(zb, zc, GD.GEOS["G1"], GD.STRIDES, form), want, bound)[0].all()
    bad = D.decode_f32(zb, zc, GD.GEOS["G1"], GD.STRIDES, form, use_max=False)
    ok, rb, rp = D.check(bad, want, bound)
    assert not np.isfinite(bad[:, :4]).all() and not ok[:, :4][~np.isfinite(bad[:, :4])].any() and rb == np.inf


# ------------------------------------------------------------------------------------------------------------------------- the sink
def sink_model(rows, last=False, merge_larger=False):
    """The SINK branch's structure on (nc, A) float32 rows: class c sits in lane group (c % 16) // 4, classes ascend within a lane (strict >
    keeps the first), then the two shuffle steps merge the four lanes (larger value wins, equal values -> smaller class).  last /
    merge_larger are the two mistakes."""
    nc, A = rows.shape
    bv, bi = np.zeros((4, A), F), -np.ones((4, A), np.int64)
    for c in range(nc):
        kg, v = (c % 16) // 4, rows[c]
        take = (bi[kg] < 0) | ((v >= bv[kg]) if last else (v > bv[kg]))
        bv[kg], bi[kg] = np.where(take, v, bv[kg]), np.where(take, c, bi[kg])
    for m in (1, 2):
        nv, ni = bv.copy(), bi.copy()
        for kg in range(4):
            ov, oi = bv[kg ^ m], bi[kg ^ m]
            take = (oi >= 0) & ((bi[kg] < 0) | (ov > bv[kg]) | ((ov == bv[kg]) & ((oi > bi[kg]) if merge_larger else (oi < bi[kg]))))
            nv[kg], ni[kg] = np.where(take, ov, bv[kg]), np.where(take, oi, bi[kg])
        bv, bi = nv, ni
    return bv[0], np.maximum(bi[0], 0)


@pytest.mark.parametrize("geo,wd", [(g_, w_) for g_ in ("G1", "G2") for w_ in GD.WIDTHS[:2]])
def test_sink_checks_reject_a_wrong_tie_rule(geo, wd):
    nc = wd[2]
    want, bound, info, zb, zc = head(geo, wd, "fp16", seed=6, tie=True)
    rows = D.decode_f32(zb, zc, GD.GEOS[geo], GD.STRIDES, "fast")[0, 4:]
    for grp in GD.TIES[nc]:                    # identical logits give identical values on a device; the restatement's random ulps do not
        for c in grp:
            rows[c] = rows[grp[0]]
    lead = np.isin(np.argmax(rows, 0), [grp[0] for grp in GD.TIES[nc]])
    assert lead.mean() > 0.5
    conf, cls = sink_model(rows)
    assert D.sink_matches_rows(conf, cls, rows)
    for kw in (dict(last=True), dict(merge_larger=True)):
        c2, k2 = sink_model(rows, **kw)
        assert np.array_equal(c2, conf) and not np.array_equal(k2, cls) and not D.sink_matches_rows(c2, k2, rows), kw
    # ... while the float64 statement alone cannot tell the members of a tie apart (which is why the GPU test has both)
    best, adm, amb = D.sink_ref(want[0, 4:], bound[0, 4:])
    assert np.take_along_axis(adm, sink_model(rows, last=True)[1][None], 0).all()
    off = conf.copy()
    off[5] = np.nextafter(off[5], F(2))
    assert not D.sink_matches_rows(off, cls, rows)


def test_sink_ref_on_a_hand_made_anchor():
    want = np.array([[0.5, 0.5, 0.5], [0.5, 0.5 + 1e-7, 0.3], [0.4, 0.4, 0.4]])
    best, adm, amb = D.sink_ref(want, np.full_like(want, 1e-6))
    assert best.tolist() == [0.5, 0.5 + 1e-7, 0.5]
    assert adm.T.tolist() == [[True, True, False], [True, True, False], [True, False, False]]
    assert amb.tolist() == [False, True, False]          # an exact tie is no ambiguity: the first-maximum rule decides it


def test_ambiguous_anchors_are_capped():
    """Over the random cases at most 0.5 % of the anchors may have more than one admissible best class (on the reference alone)."""
    for geo, wd in GEO_WIDTHS:
        for prec in ("fp16", "bf16", "fp16x3"):
            want, bound, _, _, _ = head(geo, wd, prec, seed=8)
            _, adm, amb = D.sink_ref(want[:, 4:], bound[:, 4:])
            top = np.sort(want[:, 4:], 1)
            print("%s %s %s: %d of %d anchors ambiguous; median top-two gap %.1e, median bound %.1e" % (geo, wd, prec, int(amb.sum()), amb.size, np.median(top[:, -1] - top[:, -2]), np.median(bound[:, 4:])))
            assert amb.mean() <= 0.005


# ------------------------------------------------------------------------------------------------------------------------- the plans
Z = M.ZeroWeights()


def _plan(g, prec):
    return plan(g.tables(), PREC_ID[prec], GD.BATCH)[0]


def _assert_v8_plan(g, prec, fused):
    r = _plan(g, prec)
    d = idx(g, "decode")
    src = [idx(g, "%s%d" % (n, i)) for i in range(3) for n in ("box", "cls")]
    if fused:
        assert r[d, DET_SRC:DET_SRC + 6].tolist() == src and r[src, SKIP].all() and (r[src, KERNEL] == CONV_PW).all() and r[:, SKIP].sum() == 6
    else:
        assert (r[d, DET_SRC:DET_SRC + 6] == -1).all() and not r[:, SKIP].any()


def test_every_case_graph_plans_as_its_case_says():
    seen = set()
    for cid, geo, wd, prec, fused, stress in GD.CASES:
        g = GD.head_graph(Z, GD.GEOS[geo], *wd)
        if prec != "fp32" and not fused:
            with env(ADAS_NO_DETECT_FUSE="1"):
                _assert_v8_plan(g, prec, False)
            _assert_v8_plan(g, prec, True)            # (the switch is what keeps it apart)
        else:
            _assert_v8_plan(g, prec, fused)
        seen.add((prec, fused))
    assert seen == {("fp32", False), ("fp16", True), ("bf16", True), ("fp16x3", True), ("fp16", False), ("fp16x3", False)}
    for cid, geo, wd, prec, tie in GD.SINK_CASES:
        assert (geo + "-%d.%d.%d-" % wd + prec) in [c[0] for c in GD.CASES]       # a sink case runs a graph planned above
    geo, wd = GD.NOT_FUSABLE
    for prec in ("fp16", "bf16", "fp16x3"):
        _assert_v8_plan(GD.head_graph(Z, GD.GEOS[geo], *wd), prec, False)


def test_v5_sink_graph_plans_onto_the_fused_kernel():
    g = GD.v5_graph(Z, GD.GEOS["G1"], GD.V5_NC)
    d, src = idx(g, "decode"), [idx(g, "det%d" % i) for i in range(3)]
    for prec in ("fp16", "bf16"):
        r = _plan(g, prec)
        assert r[d, DET_SRC:DET_SRC + 6].tolist() == src + [-1] * 3 and r[src, SKIP].all() and (r[src, KERNEL] == CONV_DET5).all() and r[:, SKIP].sum() == 3
