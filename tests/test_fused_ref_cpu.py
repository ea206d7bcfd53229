"""CPU tests of tests/fused_ref.py, the chain reference and bound of tests/test_gpu_fused_exact.py: the checker is judged before it judges
a kernel.  Acceptance: a float32 emulation of every fused form (torch float32 convs, float32 activation, the intermediate rounded with
storage_round) is inside the chained bound, and stays inside with every ambiguous intermediate element forced to the far end of what the
device may hold, upwards and downwards; no emulated intermediate differs from the reference's outside the ambiguous set.  Figures: the
ambiguous share and the median of (chained term / R(want)) are printed and, for the pair, held.  Mutations: the mistakes a fused launch
can make ((a) ... (h) below) are rejected in every precision the form exists in, every rejection inside the affected region, and where the
whole-tensor criterion of tests/test_gpu_conv.py / test_gpu_x3.py lets the mutated tensor through, that is asserted too.

Weak mutations: every mutation is rejected under the chained bound in every precision, but (b) -- one intermediate pixel of conv A with a
dropped tap -- only just where it is seen through the whole C2f chain: behind conv B's and cv2's chained terms 3 of the 87 elements it
reaches are out of bound in bf16, 23 of 95 in fp16, 43 of 96 in fp16x3 (worst-case terms grow by the sum of |w| with every stage: see
C2F_FIGURES).  The GPU file therefore runs conv B of the C2f launches as a probe stage (signed selection), which sees conv A's 18 x 18
region element by element, and probe weights for every other stage all the same."""
import numpy as np
import pytest

import conv_ref as CR
import fused_ref as FR
import ops_ref as R

F32 = np.float32
SILU, RELU, NONE = R.ACT_SILU, R.ACT_RELU, R.ACT_NONE
RN, RA = CR.RES_NONE, CR.RES_AFTER_ACT
P16, P3 = ("fp16", "bf16"), ("fp16", "bf16", "fp16x3")
HW, NF = (23, 37), 3          # two tile rows (16 + 7), three tile columns (16 + 16 + 5)


def _he(rng, cout, cin, k, prec):
    return CR.weights_as_stored((rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(F32), prec)


def _bias(rng, c):
    return (rng.standard_normal(c) * 0.05).astype(F32)


def _x(rng, c, hw, prec):
    return R.storage_round(rng.uniform(-2, 2, (NF, c) + hw).astype(F32), prec)


_DATA = {}


def data(form, prec):
    """The operands of one form in one precision (cached): inputs +-2, He weights stored as the engine stores them."""
    key = (form, prec)
    if key in _DATA:
        return _DATA[key]
    rng = np.random.default_rng(21)
    if form in ("pair16", "pair32"):
        c = int(form[4:])
        d = dict(x=_x(rng, c, HW, prec), w=[_he(rng, c, c, 3, prec) for _ in range(2)], b=[_bias(rng, c) for _ in range(2)])
    elif form == "c2f":
        d = dict(x=_x(rng, 32, HW, prec), w=[_he(rng, 32, 32, 1, prec), _he(rng, 16, 16, 3, prec), _he(rng, 16, 16, 3, prec), _he(rng, 32, 48, 1, prec)],
                 b=[_bias(rng, 32), _bias(rng, 16), _bias(rng, 16), _bias(rng, 32)])
    elif form == "stem2":      # 62 x 90 -> stem 31 x 45 (odd both ways) -> 16 x 23
        d = dict(x=_x(rng, 3, (62, 90), prec), w=[_he(rng, 16, 3, 3, prec), _he(rng, 32, 16, 3, prec)], b=[_bias(rng, 16), _bias(rng, 32)])
    elif form == "pool":       # 62 x 90 -> conv 31 x 45 -> pooled 16 x 23
        d = dict(x=_x(rng, 3, (62, 90), prec), w=[_he(rng, 64, 3, 7, prec)], b=[_bias(rng, 64)])
    elif form == "folded":     # x 25 x 37 (Cp 32) -> 13 x 19, t 64 channels
        d = dict(x=_x(rng, 32, (25, 37), prec), t=_x(rng, 64, (13, 19), prec), w=[_he(rng, 64, 64, 3, prec), _he(rng, 64, 32, 1, prec)],
                 b=[_bias(rng, 64), _bias(rng, 64)])
    else:
        raise ValueError(form)
    _DATA[key] = d
    return d


_REF = {}


def ref(form, prec):
    """The reference stages of a form (cached, never modified)."""
    key = (form, prec)
    if key not in _REF:
        d = data(form, prec)
        if form.startswith("pair"):
            _REF[key] = FR.pair_ref(d["x"], d["w"][0], d["b"][0], d["w"][1], d["b"][1], prec, True)
        elif form == "c2f":
            _REF[key] = FR.c2f_ref(d["x"], d["w"], d["b"], prec)
        elif form == "stem2":
            _REF[key] = FR.stem2_ref(d["x"], d["w"][0], d["b"][0], 1, d["w"][1], d["b"][1], prec)
        elif form == "pool":
            _REF[key] = (FR.stage(d["x"], d["w"][0], d["b"][0], 2, 3, RELU, prec),)
        elif form == "folded":
            _REF[key] = (FR.folded_ref(d["t"], d["w"][0], d["b"][0], d["x"], d["w"][1], d["b"][1], RELU, prec),)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------------- float32 emulation
def _f32(x, w, b, s, p, act, r=None, rm=RN):
    return CR._finish_f32(CR.acc_f32_torch(x, w, s, p), np.asarray(b, F32)[None, :, None, None], act, None if r is None else np.asarray(r, F32), rm)


def _store(st, v32, force):
    """The emulated device's store of a stage: storage_round of its own float32 value; force = +-1: every ambiguous element at the far
    end of what the bound lets the device hold (16-bit: the neighbour of the storage type that t64 +- slack1' rounds to; split precision:
    the split of t64 +- 0.95 slack1, a float32 inside the allowed interval).  Outside the ambiguous set the emulation must agree with the
    reference by itself."""
    prec = st.prec
    own = R.storage_round(v32, prec)
    t_ref, delta, amb = st.stored()
    assert np.array_equal(own[~amb].astype(np.float64), t_ref[~amb]), "a flip outside the ambiguous set"
    assert (np.abs(own - t_ref) <= delta).all()
    if force == 0:
        return own, float((own != t_ref).mean())
    if prec == "fp16x3":
        return R.storage_round((st.want + force * 0.95 * st.slack).astype(F32), prec), 1.0
    s1 = st.slack + R.EPS32 * np.abs(st.want)
    far = FR.round64(st.want + force * s1, prec).astype(F32)
    return np.where(amb, far, own), float((np.where(amb, far, own) != t_ref).mean())


def emulate(form, prec, force=0):
    """The fused form in float32 with the intermediates rounded as stored.  Returns (the output as stored, flipped share of the last
    intermediate)."""
    d, st = data(form, prec), ref(form, prec)
    w, b = d["w"], d["b"]
    if form.startswith("pair"):
        t, fl = _store(st[0], _f32(d["x"], w[0], b[0], 1, 1, SILU), force)
        return R.storage_round(_f32(t, w[1], b[1], 1, 1, SILU, d["x"], RA), prec), fl
    if form == "c2f":
        y, _ = _store(st[0], _f32(d["x"], w[0], b[0], 1, 0, SILU), force)
        y1 = np.ascontiguousarray(y[:, 16:32])
        t, fl = _store(st[1], _f32(y1, w[1], b[1], 1, 1, SILU), force)
        y2, _ = _store(st[2], _f32(t, w[2], b[2], 1, 1, SILU, y1, RA), force)
        return R.storage_round(_f32(np.concatenate([y, y2], 1), w[3], b[3], 1, 0, SILU), prec), fl
    if form == "stem2":
        t, fl = _store(st[0], _f32(d["x"], w[0], b[0], 2, 1, SILU), force)
        return R.storage_round(_f32(t, w[1], b[1], 2, 1, SILU), prec), fl
    if form == "pool":
        c = R.storage_round(_f32(d["x"], w[0], b[0], 2, 3, RELU), prec)
        return R.maxpool_ref(c, 3, 2, 1).astype(F32), 0.0
    if form == "folded":
        r32 = (CR.acc_f32_torch(d["x"], w[1], 2, 0) + b[1][None, :, None, None]).astype(F32)
        return R.storage_round(_f32(d["t"], w[0], b[0], 1, 1, RELU, r32, CR.RES_BEFORE_ACT), prec), 0.0
    raise ValueError(form)


def judge(form, prec, got):
    """(ok per element, worst |err| / bound) of an output of the form under its bound."""
    st = ref(form, prec)
    if form == "pool":
        return FR.pool_check(got, *FR.pool_interval(st[0]))
    ok, w, _ = st[-1].check(got)
    return ok, w


FORMS = [("pair16", P16), ("pair32", P16), ("c2f", P3), ("stem2", P3), ("pool", P16), ("folded", P16)]


@pytest.mark.parametrize("form,prec", [(f, p) for f, ps in FORMS for p in ps])
def test_chain_bound_accepts_the_float32_emulation(form, prec):
    """As it rounds by itself, and with every ambiguous intermediate element forced either way."""
    st = ref(form, prec)
    for s in st:
        assert s.yard[0] <= CR.YARD_CONV, (form, prec, s.yard)
    for force in ((0,) if form in ("pool", "folded") else (0, 1, -1)):
        got, flipped = emulate(form, prec, force)
        ok, w = judge(form, prec, got)
        print("%s %s force %+d: emulation's worst |err| / bound %.3f, intermediate elements that differ from the reference's %.3f %%" % (form, prec, force, w, 100 * flipped))
        assert ok.all() and w <= 1.0, (form, prec, force, int((~ok).sum()), w)
    if form not in ("pool", "folded"):
        assert w > 0.2, "the forced emulation comes within a fifth of the bound: the bound is not idle"


def _figures(st_in, st_out):
    """(ambiguous share of st_in's store, median of st_out's chained term / R(want))."""
    amb = st_in.stored()[2]
    Rw = R.store_bound(st_out.want, st_out.prec)
    return float(amb.mean()), float(np.median(st_out.chain / Rw))


@pytest.mark.parametrize("form", ["pair16", "pair32"])
@pytest.mark.parametrize("prec", P16)
def test_pair_chain_figures(form, prec):
    """The chained term of a 3x3 -> 3x3 SiLU pair stays a few half-ulps of the output: median <= 4 R(want) in fp16, <= 1 in bf16 (measured
    on the reference alone: 1.96 | 3.63 and 0.19 | 0.42 on 16 | 32 channels).  The naive form conv(R(t) + slack1, |w2|) gives 8.5 - 12.3."""
    A, B = ref(form, prec)
    share, med = _figures(A, B)
    naive = float(np.median(FR.slope(SILU) * FR.conv_abs(A.direct()[1], data(form, prec)["w"][1], 1, 1) / R.store_bound(B.want, prec)))
    print("%s %s: ambiguous %.1f %%, chained term median %.2f R(want) (naive form %.1f)" % (form, prec, 100 * share, med, naive))
    assert med <= (4.0 if prec == "fp16" else 1.0)
    assert naive > 2 * med


# the four-stage C2f chain, measured here (CPU, reference only; 23 x 37, 3 frames, inputs +-2, He weights): the ambiguous share of cv1's, conv A's
# and conv B's store, and the median chained term / R(want) of conv A, conv B and cv2.  A worst-case term grows by about the sum of |w| (13
# for a He-scaled 3x3 on 16 channels) with every stage and, once it passes a spacing, every element behind it is ambiguous: from conv B on
# the chain still holds the structure of the block (mutations (a), (c), (d), (e) below) but no longer a rounding -- the probe cases of the
# GPU file do that.  In fp16x3 R(want) is 2^-22 |want| and the term is the fp32 slack of the stages before (K_CONV 2^-24 S each).
C2F_FIGURES = {"fp16": ((0.168, 0.921, 1.0), (3.06, 47.2, 253.7)), "bf16": ((0.029, 0.412, 0.966), (0.24, 6.67, 48.9)),
               "fp16x3": ((1.0, 1.0, 1.0), (2400.0, 21699.0, 102648.0))}


@pytest.mark.parametrize("prec", P3)
def test_c2f_chain_figures(prec):
    s1, sA, sB, s2 = ref("c2f", prec)
    shares = [float(s.stored()[2].mean()) for s in (s1, sA, sB)]
    meds = [float(np.median(s.chain / R.store_bound(s.want, prec))) for s in (sA, sB, s2)]
    print("c2f %s: ambiguous cv1 %.1f %% A %.1f %% B %.1f %%;  chained term median / R(want): A %.2f  B %.2f  cv2 %.2f"
          % ((prec,) + tuple(100 * s for s in shares) + tuple(meds)))
    rs, rm = C2F_FIGURES[prec]
    assert np.allclose(shares, rs, rtol=0, atol=0.01) and np.allclose(meds, rm, rtol=0.02), "the recorded figures are the measured ones"


# ------------------------------------------------------------------------------------------------------------------------- mutations
def _c64(x, w, b, s, p, act):
    return R.act_ref(CR._conv64(x, w, b, s, p), act)


def _rnd(t, prec):
    return FR.round64(t, prec)


def _out(v64, prec):
    return R.storage_round(np.asarray(v64, np.float64).astype(F32), prec)


def _pair_parts(x, wa, ba, wb, bb, prec, mut):
    """y = SiLU(B t) + x along the reference's own path (float64, t rounded as stored), with one mutation.  Returns (y64, region)."""
    N, C, H, W = x.shape
    x = np.asarray(x, np.float64)
    t = _rnd(_c64(x, wa, ba, 1, 1, SILU), prec)
    good = _c64(t, wb, bb, 1, 1, SILU) + x
    region = np.zeros(good.shape, bool)
    if mut == "a":       # the intermediate is not zeroed outside the image: conv A is evaluated on the zero-padded window there
        te = _rnd(_c64(np.pad(x, ((0, 0), (0, 0), (2, 2), (2, 2))), wa, ba, 1, 0, SILU), prec)
        assert np.array_equal(te[:, :, 1:-1, 1:-1], t)
        bad = _c64(te, wb, bb, 1, 0, SILU) + x
        region[:, :, (0, H - 1), :] = True
        region[:, :, :, (0, W - 1)] = True
    elif mut == "b":     # tile (0, 16): the pixel (5, 15) of its 18 x 18 region (the region's left edge) is computed without the tap (1, 0)
        wd = np.asarray(wa, np.float64).copy()
        wd[:, :, 1, 0] = 0
        t2 = t.copy()
        t2[0, :, 5, 15] = _rnd(_c64(x[:1], wd, ba, 1, 1, SILU), prec)[0, :, 5, 15]
        bad = good.copy()
        bad[0, :, 4:7, 16] = (_c64(t2[:1], wb, bb, 1, 1, SILU) + x[:1])[0, :, 4:7, 16]       # (of that tile, only column 16 reads column 15)
        region[0, :, 4:7, 16] = True
    elif mut == "c":     # frame 1, tile (16, 16): the shortcut is taken from the window one pixel to the left
        bad = good.copy()
        bad[1, :, 16:, 16:32] = (good - x)[1, :, 16:, 16:32] + x[1, :, 16:, 15:31]
        region[1, :, 16:, 16:32] = True
    else:
        raise ValueError(mut)
    return good, bad, region


def mutate(form, prec, mut):
    """(good, mutated, region): the reference chain's output stored in `prec`, the same with one mistake, where the mistake can reach."""
    d = data(form, prec)
    w, b = d["w"], d["b"]
    x = np.asarray(d["x"], np.float64)
    if form.startswith("pair"):
        g, m, region = _pair_parts(x, w[0], b[0], w[1], b[1], prec, mut)
        return _out(g, prec), _out(m, prec), region
    if form == "c2f":
        y = _rnd(_c64(x, w[0], b[0], 1, 0, SILU), prec)
        y0, y1 = y[:, :16], y[:, 16:32]
        cv2 = lambda a0, a1, a2: _c64(np.concatenate([a0, a1, _rnd(a2, prec)], 1), w[3], b[3], 1, 0, SILU)
        g2, m2, reg = _pair_parts(y1, w[1], b[1], w[2], b[2], prec, mut if mut in "abc" else "c")
        good = cv2(y0, y1, g2)
        region = np.zeros(good.shape, bool)
        if mut in "abc":                                  # the Bottleneck's mistakes, seen through cv2 (a 1x1: the same pixels, every channel)
            bad = cv2(y0, y1, m2)
            region[:] = reg.any(1, keepdims=True)
        elif mut == "d":                                  # frame 2: y0 and y1 swapped in cv2's K order
            bad = good.copy()
            bad[2] = cv2(y1, y0, g2)[2]
            region[2] = True
        elif mut == "e":                                  # frame 0: the shortcut adds y0 instead of y1
            bad = good.copy()
            bad[0] = cv2(y0, y1, g2 - y1 + y0)[0]
            region[0] = True
        return _out(good, prec), _out(bad, prec), region
    if form == "stem2" and mut == "f":                    # the stem map is 31 x 45: the second conv's last row / column window ends on padding;
        t = _rnd(_c64(x, w[0], b[0], 2, 1, SILU), prec)   # the mistake reads the phantom stem column 45 (computed from the zero-extended frame)
        te = _rnd(_c64(np.pad(x, ((0, 0), (0, 0), (0, 0), (0, 2))), w[0], b[0], 2, 1, SILU), prec)
        assert te.shape[3] == t.shape[3] + 1 and np.array_equal(te[..., :-1], t)
        good = _c64(t, w[1], b[1], 2, 1, SILU)
        bad = _c64(np.pad(te, ((0, 0), (0, 0), (1, 1), (1, 0))), w[1], b[1], 2, 0, SILU)
        assert bad.shape == good.shape
        region = np.zeros(good.shape, bool)
        region[..., -1] = True
        return _out(good, prec), _out(bad, prec), region
    if form == "pool" and mut == "g":                     # conv map 31 x 45: the last pooled column's window takes the conv pixel at column 45
        c = _out(_c64(x, w[0], b[0], 2, 3, RELU), prec).astype(np.float64)
        ce = _out(_c64(np.pad(x, ((0, 0), (0, 0), (0, 0), (0, 2))), w[0], b[0], 2, 3, RELU), prec).astype(np.float64)
        assert ce.shape[3] == c.shape[3] + 1
        good = R.maxpool_ref(c, 3, 2, 1)
        bad = R.maxpool_ref(np.pad(ce, ((0, 0), (0, 0), (1, 1), (1, 0)), constant_values=-np.inf), 3, 2, 0)
        assert bad.shape == good.shape
        region = np.zeros(good.shape, bool)
        region[..., -1] = True
        return good.astype(F32), bad.astype(F32), region
    if form == "folded" and mut == "h":                   # frame 1: the projection read at x[2y + 1, 2x + 1]
        t = np.asarray(d["t"], np.float64)
        v3 = CR._conv64(t, w[0], b[0], 1, 1)
        good = R.act_ref(v3 + CR._conv64(x, w[1], b[1], 2, 0), RELU)
        xs = np.pad(x, ((0, 0), (0, 0), (0, 1), (0, 1)))[:, :, 1:, 1:]
        bad = good.copy()
        bad[1] = R.act_ref(v3 + CR._conv64(xs, w[1], b[1], 2, 0), RELU)[1]
        region = np.zeros(good.shape, bool)
        region[1] = True
        return _out(good, prec), _out(bad, prec), region
    raise ValueError((form, mut))


# mutation -> [(form, precisions)]
MUTATIONS = {
    "a": [("pair16", P16), ("pair32", P16), ("c2f", P3)],
    "b": [("pair16", P16), ("pair32", P16), ("c2f", P3)],
    "c": [("pair16", P16), ("pair32", P16), ("c2f", P3)],
    "d": [("c2f", P3)],
    "e": [("c2f", P3)],
    "f": [("stem2", P3)],
    "g": [("pool", P16)],
    "h": [("folded", P16)],
}
WEAK = {("b", "c2f")}      # rejected, but by a minority of the elements it changes: the stage has a probe case on the GPU
# where the old criterion (rel-L2 at the existing tests' tolerance, on the same tensor) lets the mutation through
OLD_BLIND = {("b", "pair16"): ("bf16",), ("b", "pair32"): P16, ("b", "c2f"): P16}


@pytest.mark.parametrize("mut,form,prec", [(m, f, p) for m, fs in MUTATIONS.items() for f, ps in fs for p in ps])
def test_chain_bound_rejects_the_mutation(mut, form, prec):
    good, bad, region = mutate(form, prec, mut)
    ok0, w0 = judge(form, prec, good)
    assert ok0.all() and w0 <= 1.0, "the reference's own chain is inside the bound"
    mutated = np.where(region, bad, good)
    assert (mutated != good).any() and np.array_equal(mutated, bad), "the mutation stays inside its region"
    ok, w = judge(form, prec, mutated)
    kind = "pair" if form.startswith("pair") else form
    rel = FR.old_rel_l2(mutated, good)
    old_pass = rel < FR.OLD_TOL[kind][prec]
    print("(%s) %s %s: %d of %d elements changed, %d rejected = %.1f %% of them (worst |err| / bound %.1f); rel-L2 %.2e -> old criterion %s"
          % (mut, form, prec, int((mutated != good).sum()), good.size, int((~ok).sum()), 100 * (~ok[mutated != good]).mean(), w, rel, "passes" if old_pass else "fails"))
    assert not ok.all(), "the chained bound must reject the mutation"
    assert ok[~region].all(), "and blame nothing outside the affected region"
    if (mut, form) not in WEAK:
        assert (~ok[mutated != good]).mean() > 0.5, "most of the elements the mistake changes are individually out of bound"
    if prec in OLD_BLIND.get((mut, form), ()):
        assert old_pass, "the whole-tensor criterion lets this mutation through: rel-L2 %.2e" % rel


# ------------------------------------------------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("prec", P3)
def test_round64_is_the_storage_rounding(prec):
    """On float32 values round64 is storage_round (one rounding of a value that needs none before it); on float64 values it rounds once:
    a value 2^-30 above a 16-bit midpoint goes up where float32 -> 16-bit (ties to even) may go down."""
    v = np.concatenate([np.random.default_rng(1).standard_normal(20000) * 3, [0.0, 6.1e-5, 3e-5, 1e-7, -2.0 ** -14, 1.0, 65000.0]]).astype(F32)
    assert np.array_equal(FR.round64(v, prec), R.storage_round(v, prec).astype(np.float64))
    if prec != "fp16x3":
        u = (R.ulp16 if prec == "fp16" else R.ulpbf)(1.0)
        assert FR.round64(1.0 + u / 2 + 2.0 ** -30, prec) == 1.0 + u and FR.round64(1.0 + u / 2, prec) == 1.0


def test_silu_slope():
    v = np.linspace(-30, 30, 2000001)
    s = 1 / (1 + np.exp(-v))
    d = s * (1 + v * (1 - s))
    assert 1.0998 < np.abs(d).max() < FR.SILU_SLOPE and abs(v[np.argmax(d)] - 2.39936) < 1e-3


def test_selection_weights_read_one_element():
    w = FR.selection(4, 3, 3, [(0, 0), (4, 1), (8, 2), (2, 0)])
    x = np.random.default_rng(2).standard_normal((1, 3, 5, 6))
    y = CR._conv64(x, w, None, 1, 1)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    assert np.array_equal(y[0, 0], xp[0, 0, 0:5, 0:6]) and np.array_equal(y[0, 1], -x[0, 1]) and np.array_equal(y[0, 2], xp[0, 2, 2:7, 2:8])
    assert np.array_equal(y[0, 3], -xp[0, 0, 0:5, 2:8])
