"""CPU tests of tests/detect56_ref.py, the per-element checker of tests/test_gpu_detect56_exact.py, and of that file's graphs.  Before a
kernel is judged: the references are the stated expressions (by hand, and against tests/graph_interp.py's torch decode of the same graphs);
the float32 restatements sit inside the bounds, closely enough to the recorded ratios; the checker REJECTS each way these kernels can go
wrong locally, in every geometry and in both sigmoid forms; a row that is out of place fails by orders of magnitude, not by a margin; the
tied pair of the sink case ties and leads on the float64 rows; and every graph of the GPU file plans onto the label its case asserts
(include/adas_hip.h adas_debug_engine_plan: no device).

What the whole-network criterion (tests/test_gpu_v6.py: boxes within atol + rtol |want|, probabilities within a flat tolerance, per
precision) lets through of the wrong kernels below, in at least one geometry -- LET_THROUGH, asserted by test_old_criterion:
    fp16 and bf16   one logit of every row moved by half an ulp of fp16 or of bf16: the mutants that stay under a pixel (0.1 px in fp16)
Everything else moves a box by a pixel or more, or a probability by more than 0.15, and fails both; the float32 modes' criterion
(1e-3 px) accepts none of them."""
import numpy as np
import pytest

import conv_ref as CR
import detect56_ref as R6
import detect_ref as D
import graph_interp
import ops_ref as R
import test_gpu_detect56_exact as G6
from test_engine_plan_cpu import BF16, CONV_DET5, DET_SRC, F16, F32, KERNEL, SKIP, X3, idx, plan

GD = G6.GD
M = G6.M
F = np.float32
PREC_ID = {"fp32": F32, "fp16": F16, "bf16": BF16, "fp16x3": X3}
GEO3 = ("G1", "G2", "G3")
STRIDES, ANCH = G6.STRIDES, G6.ANCHORS
MUT_WIDTH = (28, 288)            # no = 33, nine K steps: every wrong kernel below changes something
FAR = 100.0                      # an out-of-place row is at least this many bounds away


# ------------------------------------------------------------------------------------------------------------------------- operands
def v5_operands(geo, nc, cin, prec, seed=0, stress=False):
    """Synthetic operands of the fused head: feature maps uniform(-1, 1) rounded to the storage type, weights N(0, 1 / cin) as stored."""
    rng = np.random.default_rng(seed)
    no = nc + 5
    feats = [R.storage_round(rng.uniform(-1, 1, (G6.BATCH, cin) + hw).astype(F), prec) for hw in G6.GEOS[geo]]
    w = [(rng.standard_normal((3 * no, cin, 1, 1)) / np.sqrt(cin)).astype(F) for _ in range(3)]
    b = [(rng.standard_normal(3 * no) * 0.05).astype(F) for _ in range(3)]
    if stress:
        w, b = [(a * 40).astype(F) for a in w], [np.linspace(-60, 60, 3 * no).astype(F) for _ in range(3)]
    return feats, [CR.weights_as_stored(a, prec) for a in w], b


def v5_case(geo, nc, cin, form, prec="fp16", **kw):
    """(want, bound, the float32 logits, the operands) of a synthetic case in one form: the fast form is the fused head, the exact form
    detect_v5_kernel on the float32 logits of the same operands."""
    ops = v5_operands(geo, nc, cin, prec, **kw)
    info = {}
    want, bound = R6.v5_head_ref(*ops, G6.GEOS[geo], STRIDES, ANCH, prec, info=info)
    z32 = [z.astype(F) for z in info["z"]]
    if form == "exact":
        want, bound = R6.v5_ref([z.astype(np.float64) for z in z32], None, G6.GEOS[geo], STRIDES, ANCH, "exact")
    return want, bound, z32, ops, info


def v6_operands(geo, nc, dfl, seed=0, kind=None):
    """Synthetic float32 operands of a v6 head: reg and class logits N(0, 2)."""
    rng = np.random.default_rng(seed)
    nreg = 68 if dfl else 4
    reg = [rng.normal(0, 2, (G6.BATCH, nreg) + hw).astype(F) for hw in G6.GEOS[geo]]
    cls = [rng.normal(0, 2, (G6.BATCH, nc) + hw).astype(F) for hw in G6.GEOS[geo]]
    if kind == "stress":
        reg = [(r * 40 + np.tile(np.linspace(-60, 60, 17), 4)[None, :, None, None]).astype(F) for r in reg]
    if kind == "argmax":
        for r in reg:
            r[:, 0] += 30
            r[:, 2 * 17 + 16] += 30
    if kind == "equal":
        reg = [np.full_like(r, 1.5) for r in reg]
    return reg, cls


# ------------------------------------------------------------------------------------------------------------------------- the references
def test_v5_reference_is_the_expression_written_out():
    """One element per column by hand: scalar Python on the stated formulas and the stated row order."""
    sizes = G6.GEOS["G3"]
    rng = np.random.default_rng(1)
    no = 9
    z = [rng.normal(0, 3, (2, 3 * no, h * w)) for h, w in sizes]
    want, bound = R6.v5_ref(z, None, sizes, STRIDES, ANCH, "fast")
    l, a, y, x, b = 1, 2, 4, 5, 1
    hw = [h * w for h, w in sizes]
    row = 3 * hw[0] + a * hw[1] + y * sizes[1][1] + x
    s = [1 / (1 + np.exp(-z[l][b, a * no + c, y * sizes[1][1] + x])) for c in range(no)]
    exp = [(2 * s[0] - 0.5 + x) * 16, (2 * s[1] - 0.5 + y) * 16, (2 * s[2]) ** 2 * ANCH[l * 6 + a * 2], (2 * s[3]) ** 2 * ANCH[l * 6 + a * 2 + 1]] + s[4:]
    assert want.shape == (2, 3 * sum(hw), no) and np.allclose(want[b, row], exp, rtol=0, atol=1e-11) and (bound > 0).all()


def test_v6_reference_is_the_expression_written_out():
    sizes = G6.GEOS["G1"]
    rng = np.random.default_rng(2)
    for dfl in (False, True):
        reg = [rng.normal(0, 2, (2, 68 if dfl else 4, h, w)).astype(F) for h, w in sizes]
        cls = [rng.normal(0, 2, (2, 3, h, w)).astype(F) for h, w in sizes]
        want, bound = R6.v6_ref(reg, cls, sizes, STRIDES, dfl)
        l, y, x, b = 2, 1, 3, 1
        row = 117 + 35 + y * 4 + x
        r = reg[l][b, :, y, x].astype(np.float64)
        d = [float((np.exp(r[17 * k:17 * k + 17]) * np.arange(17)).sum() / np.exp(r[17 * k:17 * k + 17]).sum()) for k in range(4)] if dfl else list(r)
        x1, y1, x2, y2 = x + 0.5 - d[0], y + 0.5 - d[1], x + 0.5 + d[2], y + 0.5 + d[3]
        exp = [(x1 + x2) / 2 * 32, (y1 + y2) / 2 * 32, (x2 - x1) * 32, (y2 - y1) * 32, 1.0] + [1 / (1 + np.exp(-float(c))) for c in cls[l][b, :, y, x]]
        assert want.shape == (2, 164, 8) and np.allclose(want[b, row], exp, rtol=0, atol=1e-10)
        assert (bound[..., 4] == 0).all() and (np.delete(bound, 4, 2) > 0).all()


def test_references_agree_with_the_graph_interpreter():
    """The GPU file's graphs through tests/graph_interp.py (torch float32: its own decode of OP_DETECT_V5 / V6 from the builders' tables)
    against the float64 references on the interpreter's own logits: inside twice the exact-form bound plus torch's own float32 pow."""
    x = GD.frames(G6.GEOS["G3"][0])
    g, _ = G6.fused_graph("G3", 28, 32)
    taps = {}
    got = graph_interp.run(g, x, taps)[0]
    want, bound = R6.v5_logits_ref([taps["det%d" % i] for i in range(3)], G6.GEOS["G3"], STRIDES, ANCH)
    assert R6.check(got, want, 4 * bound)[0].all()
    g, _ = G6.v6_case_graph(False, "G3", 3)
    taps = {}
    got = graph_interp.run(g, x, taps)[0]
    want, bound = R6.v6_ref([taps["reg%d" % i] for i in range(3)], [taps["cls%d" % i] for i in range(3)], G6.GEOS["G3"], STRIDES, False)
    assert R6.check(got, want, 4 * bound)[0].all()


# ------------------------------------------------------------------------------------------------------------------------- the restatements
def test_restatements_sit_inside_the_bound():
    """v5_f32 in both forms and v6_f32 with and without DFL on every geometry and width and on the stress / argmax / equal operands:
    inside the bound, and the worst ratios are the ones detect56_ref records (held to within 15 % below)."""
    worst = {k: [0.0, 0.0] for k in R6.YARD56}

    def note(key, r):
        worst[key] = [max(worst[key][0], r[0]), max(worst[key][1], r[1])]

    for geo in GEO3:
        widths = G6.FUSED_WIDTHS if geo == "G3" else (G6.FUSED_WIDTHS[0], G6.FUSED_WIDTHS[3])
        for (nc, cin), stress in [(w_, False) for w_ in widths] + ([((11, 32), True)] if geo == "G1" else []):
            for prec in ("fp16", "bf16"):
                info = v5_case(geo, nc, cin, "fast", prec, seed=3, stress=stress)[4]
                if stress:
                    assert info["min_z"] <= -G6.OVERFLOW_Z and info["max_z"] >= G6.OVERFLOW_Z
                for seed in range(2):
                    note("v5-fast", R6.v5_yardstick(info["z"], G6.GEOS[geo], STRIDES, ANCH, "fast", seed))
                    note("v5-exact", R6.v5_yardstick([z.astype(F) for z in info["z"]], G6.GEOS[geo], STRIDES, ANCH, "exact", seed))
        for dfl in (False, True):
            for nc, kind in [(n_, None) for n_ in G6.V6_NCS] + ([(80, k) for k in G6.DFL_OVER] if dfl else []):
                reg, cls = v6_operands(geo, nc, dfl, seed=3, kind=kind)
                for seed in range(2):
                    note("v6-dfl" if dfl else "v6", R6.v6_yardstick(reg, cls, G6.GEOS[geo], STRIDES, dfl, seed))
    print("decode restatements, worst |f32 - f64| / bound: " + "  ".join("%s box %.3f other %.3f" % (k, v[0], v[1]) for k, v in worst.items()))
    for k in worst:
        for got, rec in zip(worst[k], R6.YARD56[k]):
            assert 0.85 * rec <= got <= rec <= 1.0, (k, worst[k], R6.YARD56[k])


def test_restatement_covers_whole_fused_head():
    """With the float32 conv in front (torch float32 conv2d on the same operands) the restatement sits inside the fused head's bound."""
    for prec in ("fp16", "bf16"):
        for nc, cin in ((28, 288), (91, 512)):
            want, bound, _, (feats, w, b), _ = v5_case("G3", nc, cin, "fast", prec, seed=5)
            z32 = [(CR.acc_f32_torch(feats[l], w[l], 1, 0) + b[l][None, :, None, None]).astype(F).reshape(G6.BATCH, 3 * (nc + 5), -1) for l in range(3)]
            ok, rb, rp = R6.check(R6.v5_f32(z32, G6.GEOS["G3"], STRIDES, ANCH, "fast"), want, bound)
            print("float32 v5 head %s (%d, %d): worst |f32 - f64| / bound box %.3f other %.3f" % (prec, nc, cin, rb, rp))
            assert ok.all()


# ------------------------------------------------------------------------------------------------------------------------- wrong kernels, v5
def _hw_off5(geo):
    hw = R6.cells(G6.GEOS[geo])
    return hw, R6.v5_row_off(G6.GEOS[geo])


def _cell_major(out, geo, **_):
    hw, off = _hw_off5(geo)
    for l in range(3):
        blk = out[:, off[l]:off[l] + 3 * hw[l]].copy()
        out[:, off[l]:off[l] + 3 * hw[l]] = blk.reshape(blk.shape[0], 3, hw[l], -1).transpose(0, 2, 1, 3).reshape(blk.shape)
    return out


def _row_off_by_one(out, geo, **_):
    hw, off = _hw_off5(geo)
    blk = out[:, off[1]:off[1] + 3 * hw[1]].copy()
    out[:, off[1]] = 0
    out[:, off[1] + 1:off[1] + 1 + 3 * hw[1]] = blk
    return out


def _frames_swapped(out, geo, **_):
    return out[[1, 0, 2]]


def _last_block_unwritten(out, geo, **_):
    hw, off = _hw_off5(geo)
    out[:, off[0] + 2 * hw[0] + (hw[0] - 1) // 128 * 128:off[0] + 3 * hw[0]] = 0          # level 0, anchor 2, its last 128-cell block
    return out


def _second_pass_unwritten(out, geo, **_):
    B, A, no = out.shape
    flat = out[:, :32].reshape(B, -1).copy()                                              # level 0, anchor 0, wave 0: 32 rows, 32 no elements
    flat[:, 512:1024] = 0
    out[:, :32] = flat.reshape(B, 32, no)
    return out


def _k_delta(ops, lo, hi):
    """The part of every logit that the channels lo .. hi - 1 contribute, float32 (B, 3 no, hw) per level."""
    feats, w, _ = ops
    return [CR._conv64(f[:, lo:hi], w_[:, lo:hi], None, 1, 0).reshape(f.shape[0], w_.shape[0], -1).astype(F) for f, w_ in zip(feats, w)]


def _last_k_dropped(z, ops, **_):
    cin = ops[0][0].shape[1]
    return [(a - d).astype(F) for a, d in zip(z, _k_delta(ops, cin - 32, cin))]


def _chunk2_first_k_doubled(z, ops, **_):
    assert ops[0][0].shape[1] > 256
    return [(a + d).astype(F) for a, d in zip(z, _k_delta(ops, 256, 288))]


def _padded_tile_stride(z, ops, **_):
    """pack_weights_det5_kernel reading row a (16 NT) + c instead of a no + c: an anchor's rows slide into the next anchor's (zero past the
    last row), the biases stay."""
    feats, w, b = ops
    out = []
    for f, w_, b_ in zip(feats, w, b):
        no = w_.shape[0] // 3
        src = np.concatenate([w_, np.zeros((48, ) + w_.shape[1:], w_.dtype)], 0)
        rows = np.asarray([a * 16 * ((no + 15) // 16) + c for a in range(3) for c in range(no)])
        out.append((CR._conv64(f, src[rows], None, 1, 0) + b_[None, :, None, None].astype(np.float64)).reshape(f.shape[0], 3 * no, -1).astype(F))
    return out


def _half_ulp_every_row(prec):
    def f(z, ops, geo, **_):
        """Per row of the head the logit nearest +-1 moved up by half an ulp of the storage type at its magnitude."""
        out = []
        for a in z:
            B, c, hw = a.shape
            no = c // 3
            v = a.reshape(B, 3, no, hw).copy()
            i = np.abs(np.abs(v) - 1.0).argmin(2)
            pick = np.take_along_axis(v, i[:, :, None], 2)
            assert (np.abs(pick) > 0.5).all() and (np.abs(pick) < 2).all()
            step = np.exp2(np.floor(np.log2(np.abs(pick))) - (11 if prec == "fp16" else 8)).astype(F)
            np.put_along_axis(v, i[:, :, None], (pick + step).astype(F), 2)
            out.append(v.reshape(B, c, hw))
        return out
    return f


A3 = np.asarray(ANCH, F).reshape(3, 3, 2)
# name -> (on the logits (fused form only), keyword arguments of v5_f32, on the output, an out-of-place row)
WRONG5 = {
    "anchor-w-h-swapped": (None, dict(anchors=A3[..., ::-1]), None, False),
    "neighbour-levels-anchors": (None, dict(anchors=np.roll(A3, 1, 0)), None, False),
    "anchor-a+1": (None, dict(anchors=np.roll(A3, -1, 1)), None, False),
    "grid-x-y-swapped": (None, dict(swap_xy=True), None, False),
    "0.5-dropped": (None, dict(half=0.0), None, False),
    "neighbour-levels-stride": (None, dict(strides=(16, 8, 16)), None, False),
    "cell-major-rows": (None, {}, _cell_major, True),
    "row_off-off-by-one": (None, {}, _row_off_by_one, True),
    "frames-swapped": (None, {}, _frames_swapped, False),
    "last-block-unwritten": (None, {}, _last_block_unwritten, True),
    "second-store-pass-unwritten": (None, {}, _second_pass_unwritten, True),
    "last-k-step-dropped": (_last_k_dropped, {}, None, False),
    "chunk-2-first-k-step-doubled": (_chunk2_first_k_doubled, {}, None, False),
    "padded-tile-row-of-next-anchor": (_padded_tile_stride, {}, None, False),
    "half-ulp-fp16-every-row": (_half_ulp_every_row("fp16"), {}, None, False),
    "half-ulp-bf16-every-row": (_half_ulp_every_row("bf16"), {}, None, False),
}


def _wrong5(name, geo, form):
    """(good, bad, want, bound, prec) of one wrong v5 kernel, or None where it does not exist (a logit mutation of the exact form)."""
    on_logits, kw, on_output, _ = WRONG5[name]
    if on_logits is not None and form == "exact":
        return None
    prec = "bf16" if "bf16" in name else "fp16"
    nc, cin = MUT_WIDTH
    want, bound, z32, ops, _ = v5_case(geo, nc, cin, form, prec, seed=2)
    kw = dict(kw)
    strides, anchors = kw.pop("strides", STRIDES), kw.pop("anchors", ANCH)
    good = R6.v5_f32(z32, G6.GEOS[geo], STRIDES, ANCH, form)
    bad = R6.v5_f32(on_logits([z.copy() for z in z32], ops, geo=geo) if on_logits else z32, G6.GEOS[geo], strides, anchors, form, **kw)
    if on_output:
        bad = on_output(bad.copy(), geo)
    return good, bad, want, bound, prec


@pytest.mark.parametrize("form", R6.FORMS)
@pytest.mark.parametrize("geo", GEO3)
@pytest.mark.parametrize("name", list(WRONG5))
def test_wrong_v5_kernels_are_rejected(name, geo, form):
    r = _wrong5(name, geo, form)
    if r is None:
        return
    good, bad, want, bound, prec = r
    ok, rb, rp = R6.check(good, want, bound)
    assert ok.all() and max(rb, rp) <= 1.0
    assert not np.array_equal(bad, good), "the mutation changes nothing"
    ok, rb, rp = R6.check(bad, want, bound)
    print("%s %s %s: |err| / bound box %.3g other %.3g" % (name, geo, form, rb, rp))
    assert not ok.all()
    if WRONG5[name][3]:
        assert max(rb, rp) >= FAR, "an out-of-place row fails outright"
    if "half-ulp" in name:          # every row notices its one moved logit, several bounds away
        assert (~ok).any(2).all() and R6.ratios(bad, want, bound).max(2).min() > 4


# ------------------------------------------------------------------------------------------------------------------------- wrong kernels, v6
# name -> (keyword arguments of v6_f32, DFL only, the operands' kind, geometries where it changes nothing)
WRONG6 = {
    "anchor-without-0.5": (dict(half=0.0), False, None, ()),
    "ltrb-read-as-tlbr": (dict(order=(1, 0, 3, 2)), False, None, ()),
    "xyxy-emitted": (dict(xyxy=True), False, None, ()),
    "objectness-not-1": (dict(obj=np.nextafter(F(1), F(0))), False, None, ()),
    "straddling-block-takes-first-rows-level": (dict(first_row_level=True), False, None, ("G2",)),
    "bins-weighted-i+1": (dict(bins=np.arange(1, 18)), True, None, ()),
    "16-bins": (dict(nbins=16), True, None, ()),
    "side-stride-16": (dict(side_stride=16), True, None, ()),
    "no-max-subtraction": (dict(use_max=False), True, "stress", ()),
}


@pytest.mark.parametrize("dfl", [False, True], ids=["plain", "dfl"])
@pytest.mark.parametrize("geo", GEO3)
@pytest.mark.parametrize("name", list(WRONG6))
def test_wrong_v6_kernels_are_rejected(name, geo, dfl):
    kw, dfl_only, kind, vacuous = WRONG6[name]
    if dfl_only and not dfl:
        return
    for nc in (20, 1):
        reg, cls = v6_operands(geo, nc, dfl, seed=2, kind=kind)
        want, bound = R6.v6_ref(reg, cls, G6.GEOS[geo], STRIDES, dfl)
        good = R6.v6_f32(reg, cls, G6.GEOS[geo], STRIDES, dfl)
        ok, rb, rp = R6.check(good, want, bound)
        assert ok.all() and max(rb, rp) <= 1.0
        bad = R6.v6_f32(reg, cls, G6.GEOS[geo], STRIDES, dfl, **kw)
        if geo in vacuous:                   # G2's level boundaries are block boundaries: no block straddles
            assert np.array_equal(bad, good, equal_nan=True)
            continue
        ok, rb, rp = R6.check(bad, want, bound)
        print("%s %s nc %d: |err| / bound box %.3g other %.3g" % (name, geo, nc, rb, rp))
        assert not ok.all()
        if name == "objectness-not-1":
            assert rp == np.inf and not ok[..., 4].any()
        if name == "no-max-subtraction":
            assert max(float(np.abs(r).max()) for r in reg) >= 100 and not np.isfinite(bad[..., :4]).all()


def test_equal_logits_give_distance_8():
    reg, cls = v6_operands("G1", 3, True, kind="equal")
    want, bound = R6.v6_ref(reg, cls, G6.GEOS["G1"], STRIDES, True)
    st = np.concatenate([np.full(h * w, float(s)) for (h, w), s in zip(G6.GEOS["G1"], STRIDES)])
    assert np.abs(want[..., 2] - 16 * st).max() < 1e-9 and (bound[..., 2] < 1e-4 * st).all()          # 8 to within 10^-4 grid units


# ------------------------------------------------------------------------------------------------------------------------- the old criterion
LET_THROUGH = {("half-ulp-fp16-every-row", "fp16"), ("half-ulp-fp16-every-row", "bf16"), ("half-ulp-bf16-every-row", "fp16"), ("half-ulp-bf16-every-row", "bf16")}


def test_old_criterion():
    """Which (wrong kernel, precision) pairs the whole-network criterion accepts in at least one geometry, judged against float64 with
    nothing else wrong: exactly the module docstring's list.  (The criterion of the float32 modes accepts none.)"""
    through = set()
    for name in WRONG5:
        for geo in GEO3:
            for form, precs in (("fast", ("fp16", "bf16")), ("exact", ("fp32", "fp16x3"))):
                r = _wrong5(name, geo, form)
                if r is None:
                    continue
                _, bad, want, _, _ = r
                through |= {(name, p) for p in precs if R6.old_criterion(bad, want, p)}
    for name, (kw, dfl_only, kind, vacuous) in WRONG6.items():
        for geo in GEO3:
            if geo in vacuous:
                continue
            for dfl in ((True,) if dfl_only else (False, True)):
                reg, cls = v6_operands(geo, 20, dfl, seed=2, kind=kind)
                want, _ = R6.v6_ref(reg, cls, G6.GEOS[geo], STRIDES, dfl)
                bad = R6.v6_f32(reg, cls, G6.GEOS[geo], STRIDES, dfl, **kw)
                through |= {(name, p) for p in G6.PRECS if R6.old_criterion(bad, want, p, obj_one=True)}
    print("the whole-network criterion lets through:", sorted(through))
    assert through == LET_THROUGH, sorted(through ^ LET_THROUGH)


# ------------------------------------------------------------------------------------------------------------------------- the tie assumption
def test_sink_pair_ties_and_leads_on_the_float64_rows():
    """The sink case's graph on the CPU (tests/graph_interp.py gives the float32 logits, detect56_ref the float64 rows): the pair's two
    class columns are equal on every row and their product with the objectness is the row's largest on more than half of the rows."""
    nc, cin = G6.SINK_WIDTH
    g, _ = G6.fused_graph(G6.SINK_GEO, nc, cin, "tie")
    taps = {}
    graph_interp.run(g, GD.frames(G6.GEOS[G6.SINK_GEO][0]), taps)
    want, _ = R6.v5_logits_ref([taps["det%d" % i] for i in range(3)], G6.GEOS[G6.SINK_GEO], STRIDES, ANCH)
    p0, p1 = G6.SINK_PAIR
    prod = want[..., 5:] * want[..., 4:5]
    lead = np.argmax(prod, -1) == p0
    print("sink pair %s on the float64 rows: leads on %d of %d" % (G6.SINK_PAIR, int(lead.sum()), lead.size))
    assert np.array_equal(want[..., 5 + p0], want[..., 5 + p1]) and lead.mean() > 0.5


# ------------------------------------------------------------------------------------------------------------------------- the plans
Z = M.ZeroWeights()


def _label(g, prec):
    """The decode's label as csrc/engine_schedule.cpp layer_label derives it from the plan's rows, and the rows."""
    r = plan(g.tables(), PREC_ID[prec], G6.BATCH)[0]
    d = idx(g, "decode")
    op = g.ops[d]
    if op["type"] == M.OP_DETECT_V5:
        return ("detect_v5_fused_kernel" if r[d, DET_SRC] >= 0 else "detect_v5_kernel"), r
    assert op["type"] == M.OP_DETECT_V6
    return ("detect_v6_dfl_kernel" if len(op["params"]) > 5 and op["params"][5] != 0 else "detect_v6_kernel"), r


def _assert_v5_plan(g, prec, fused):
    label, r = _label(g, prec)
    d, src = idx(g, "decode"), [idx(g, "det%d" % i) for i in range(3)]
    if fused:
        assert label == "detect_v5_fused_kernel" and r[d, DET_SRC:DET_SRC + 6].tolist() == src + [-1] * 3
        assert r[src, SKIP].all() and (r[src, KERNEL] == CONV_DET5).all() and r[:, SKIP].sum() == 3
    else:
        assert label == "detect_v5_kernel" and (r[d, DET_SRC:DET_SRC + 6] == -1).all() and not r[:, SKIP].any()


def test_every_case_graph_plans_as_its_case_says():
    for cid, geo, nc, cin, prec, kind in G6.FUSED_CASES:
        _assert_v5_plan(G6.v5_graph(Z, G6.GEOS[geo], nc, cin, sliced=kind == "slice"), prec, True)
    assert {c[5] for c in G6.FUSED_CASES} == {None, "slice", "stress"}
    for prec in ("fp16", "bf16"):
        _assert_v5_plan(G6.v5_graph(Z, G6.GEOS[G6.SINK_GEO], *G6.SINK_WIDTH), prec, True)
    for cid, geo, nc, prec in G6.PLAIN_CASES:
        _assert_v5_plan(G6.v5_graph(Z, G6.GEOS[geo], nc), prec, False)
    assert ("G1", 92, "fp16") in [c[1:] for c in G6.PLAIN_CASES]          # no = 97 does not fuse, while no = 96 does
    _assert_v5_plan(G6.v5_graph(Z, G6.GEOS["G1"], 91), "fp16", True)
    for cid, dfl, geo, nc, prec, kind in G6.V6_CASES:
        label, r = _label(G6.v6_graph(Z, G6.GEOS[geo], nc, dfl, wide=kind == "wide"), prec)
        assert label == ("detect_v6_dfl_kernel" if dfl else "detect_v6_kernel") and not r[:, SKIP].any(), cid
