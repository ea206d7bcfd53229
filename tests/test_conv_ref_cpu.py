"""CPU tests of tests/conv_ref.py, the per-element checker of tests/test_gpu_conv_exact.py.  Three things have to hold before a kernel is
judged by it: the recorded yardstick covers the float32 restatements it is derived from (and closely); the activation term A covers
NumPy restatements of the three SiLU forms with their hardware steps moved by +-1 ulp; and the checker REJECTS the local mistakes a conv
kernel can make -- each of which the whole-tensor criterion of tests/test_gpu_conv.py / test_gpu_x3.py (rel-L2 at 1e-2 / 1.5e-3) lets
through, asserted on the same mutated tensor -- while it accepts every correctly rounded store, a tie rounded either way included."""
import numpy as np
import pytest

import conv_ref as CR
import ops_ref as R
from test_x3_silu_model import x3_silu_model

F32 = np.float32


def _layer(rng, prec, cin, cout, k, s, hw, act, res_mode, batch=3):
    """A synthetic layer of the GPU cases' distributions: signed operands a few units wide, He-scaled weights, stored in `prec`."""
    H, W = hw
    p = k // 2
    x = R.storage_round(rng.standard_normal((batch, cin, H, W)).astype(F32), prec)
    w = CR.weights_as_stored((rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(F32), prec)
    b = (rng.standard_normal(cout) * 0.05).astype(F32)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    r = None if res_mode == CR.RES_NONE else R.storage_round(rng.standard_normal((batch, cout, Ho, Wo)).astype(F32), prec)
    return x, w, b, s, p, act, r, res_mode


# ------------------------------------------------------------------------------------------------------------------------- yardstick
YARD_LAYERS = [   # cin, k, map: K = 9 * 16 ... 9 * 512 and 1 * 2048, and the short sums of the pointwise, stem and generic cases (K = 16, 40, 27, 147, 108, 72, 200)
    (16, 3, (12, 20)), (32, 3, (12, 20)), (64, 3, (12, 20)), (128, 3, (10, 12)), (256, 3, (6, 10)), (512, 3, (6, 10)), (2048, 1, (6, 10)),
    (16, 1, (48, 80)), (40, 1, (48, 80)), (3, 3, (48, 80)), (3, 7, (48, 80)), (3, 6, (48, 80)), (8, 3, (48, 80)), (8, 5, (48, 80)),     # (large maps: the worst of more elements)
]
YARD_EPILOGUES = [(R.ACT_NONE, CR.RES_NONE), (R.ACT_SILU, CR.RES_NONE), (R.ACT_RELU, CR.RES_BEFORE_ACT), (R.ACT_LEAKY, CR.RES_AFTER_ACT),
                  (R.ACT_SILU, CR.RES_AFTER_ACT), (R.ACT_SILU, CR.RES_BEFORE_ACT)]


def test_yardstick_constant_covers_the_float32_restatements():
    """K_CONV = max(4, 4 * worst |f32 - f64| / (2^-24 S)) over torch's float32 conv2d and the sequential float32 accumulation, on
    synthetic layers in all four storage roundings with every epilogue.  The figures printed here stand next to YARD_CONV."""
    rng = np.random.default_rng(7)
    worst_t = worst_s = 0.0
    per_k = {}
    for cin, k, hw in YARD_LAYERS:
        for prec in R.PRECISIONS:
            x, w, b, s, p, _, r, _ = _layer(rng, prec, cin, 32, k, 1, hw, R.ACT_NONE, CR.RES_AFTER_ACT)
            sums = CR.conv_sums64(x, w, s, p)          # (the sums are shared by the six epilogues)
            accs = CR.conv_accs_f32(x, w, s, p, sums[0].shape)
            for act, rm in YARD_EPILOGUES:
                rr = None if rm == CR.RES_NONE else r
                want, S, v = CR.layer_from_sums(sums, b, act, rr, rm)
                y, yt, ys = CR.yardstick_from_accs(accs, b, act, rr, rm, want, S)
                worst_t, worst_s = max(worst_t, yt), max(worst_s, ys)
                per_k[cin * k * k] = max(per_k.get(cin * k * k, 0.0), y)
    print("conv yardstick ratios: torch float32 conv2d %.3f  sequential %.3f;  per K: %s"
          % (worst_t, worst_s, "  ".join("%d: %.2f" % kv for kv in sorted(per_k.items()))))
    worst = max(worst_t, worst_s)
    assert 0.85 * CR.YARD_CONV <= worst <= CR.YARD_CONV, (worst, CR.YARD_CONV)     # the recorded worst ratio covers these layers, and closely
    assert CR.K_CONV == max(4.0, 4 * CR.YARD_CONV)                                   # the rule, nothing added


def test_sequential_restatement_is_the_plain_loop():
    """acc_f32_seq (with the float32 epilogue behind it) against a scalar Python loop in the stated order (tap-major, channel-minor) on a handful of elements, and
    both restatements against float64 within a few roundings."""
    rng = np.random.default_rng(1)
    x, w, b, s, p, act, r, rm = _layer(rng, "fp16", 8, 4, 3, 2, (7, 9), R.ACT_LEAKY, CR.RES_BEFORE_ACT)
    want, S, v = CR.conv_layer_ref(x, w, b, s, p, act, r, rm)
    idx = CR.sample_index(want.shape)
    assert len(idx[0]) == want.size                   # a small output is taken whole
    b4 = b[None, :, None, None]
    seq = CR._finish_f32(CR.acc_f32_seq(x, w, s, p, idx).reshape(want.shape), b4, act, r, rm)
    for n, co, oy, ox in ((0, 0, 0, 0), (2, 3, 3, 4), (1, 2, 0, 4), (1, 1, 3, 0)):
        acc = F32(0)
        for i in range(3):
            for j in range(3):
                for c in range(8):
                    iy, ix = oy * s + i - p, ox * s + j - p
                    if 0 <= iy < 7 and 0 <= ix < 9:
                        acc = F32(acc + F32(x[n, c, iy, ix] * w[co, c, i, j]))
        u = F32(F32(acc + b[co]) + r[n, co, oy, ox])
        assert seq[n, co, oy, ox] == np.maximum(u, F32(0.1) * u)
    assert np.abs(seq - want).max() <= 16 * R.EPS32 * S.max()
    assert np.abs(CR._finish_f32(CR.acc_f32_torch(x, w, s, p), b4, act, r, rm) - want).max() <= 16 * R.EPS32 * S.max()
    assert CR.conv_yardstick(x, w, b, s, p, act, r, rm, want, S)[0] <= CR.YARD_CONV
    assert len(CR.sample_index((3, 64, 40, 56))[0]) == CR.YARD_SAMPLE >= 4096


def test_reference_is_the_layer_expression():
    """conv_layer_ref against the expression written out with einsum, both residual modes; S is the same sum on magnitudes."""
    rng = np.random.default_rng(2)
    x, w, b = rng.standard_normal((2, 5, 6, 7)), rng.standard_normal((4, 5, 3, 3)), rng.standard_normal(4)
    r = rng.standard_normal((2, 4, 6, 7))
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    v = sum(np.einsum("nchw,oc->nohw", xp[:, :, i:i + 6, j:j + 7], w[:, :, i, j]) for i in range(3) for j in range(3)) + b[None, :, None, None]
    silu = lambda t: t / (1 + np.exp(-t))
    want, S, pre = CR.conv_layer_ref(x, w, b, 1, 1, R.ACT_SILU, r, CR.RES_AFTER_ACT)
    assert np.allclose(want, silu(v) + r, rtol=0, atol=1e-13) and np.allclose(pre, v, rtol=0, atol=1e-13)
    want, S, pre = CR.conv_layer_ref(x, w, b, 1, 1, R.ACT_SILU, r, CR.RES_BEFORE_ACT)
    assert np.allclose(want, silu(v + r), rtol=0, atol=1e-13) and np.allclose(pre, v + r, rtol=0, atol=1e-13)
    Sw = sum(np.einsum("nchw,oc->nohw", np.abs(xp[:, :, i:i + 6, j:j + 7]), np.abs(w[:, :, i, j])) for i in range(3) for j in range(3))
    assert np.allclose(S, Sw + np.abs(b)[None, :, None, None] + np.abs(r), rtol=0, atol=1e-13) and (S >= np.abs(pre) - 1e-12).all()


# ------------------------------------------------------------------------------------------------------------------------- A(prec, act)
def _within_one_ulp(exact64, rng):
    """A float32 result with an error below 1 ulp: one of the two float32 neighbours of the exact value, picked at random per element
    (what "accurate to 1 ulp" allows a hardware exp2 / rcp and a library expf to return)."""
    with np.errstate(over="ignore", under="ignore"):
        near = np.asarray(exact64, np.float64).astype(F32)
    below = np.where(near.astype(np.float64) > exact64, np.nextafter(near, F32(-np.inf)), near).astype(F32)
    above = np.where(below.astype(np.float64) < exact64, np.nextafter(below, F32(np.inf)), below).astype(F32)
    return np.where(rng.integers(0, 2, near.shape) == 1, above, below).astype(F32)


def _silu_inputs():
    rng = np.random.default_rng(3)
    return np.concatenate([rng.normal(0, 3, 400000), rng.uniform(-80, 80, 300000), rng.normal(0, 0.1, 100000),
                           np.array([0.0, 1e-30, -1e-30, 80.0, -80.0, 20.0, -20.0])]).astype(F32)


def test_silu_term_covers_the_16_bit_form():
    """v * rcp(1 + exp2(fl(-v * log2 e))) in NumPy float32 with exp2 and rcp off by up to 1 ulp either way (v_exp_f32, v_rcp_f32 at their
    documented accuracy: either float32 neighbour of the exact result): inside A for every value, and A is far below the 16-bit store's half ulp."""
    rng = np.random.default_rng(4)
    v = _silu_inputs()
    t = (-v * F32(1.4426950408889634)).astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        e = _within_one_ulp(np.exp2(t.astype(np.float64)), rng)
        q = _within_one_ulp(1.0 / (F32(1) + e).astype(F32).astype(np.float64), rng)
    got = (v * q).astype(F32)
    want = R.act_ref(v, R.ACT_SILU)
    for prec in ("fp16", "bf16"):
        A = CR.act_slack(v.astype(np.float64), prec, R.ACT_SILU)
        err = np.abs(got.astype(np.float64) - want)
        nz = A > 0
        print("SiLU %s: worst |err| / A %.3f" % (prec, (err[nz] / A[nz]).max()))
        assert (err <= A).all() and (err[nz] / A[nz]).max() > 0.2          # covered, and not by a mile
        Rb = R.store_bound(want, prec)                                       # far below half an ulp of the storage type: a 50th up to |v| = 20, a 20th at 80
        assert (A <= Rb / 20).all() and (A[np.abs(v) <= 20] <= Rb[np.abs(v) <= 20] / 50).all()


def test_silu_term_covers_the_fp32_and_the_split_form():
    """v / (1 + expf(-v)) with expf off by up to 1 ulp either way and a correctly rounded division; x3_silu as
    tests/test_x3_silu_model.py restates it, with its 1-ulp noise on exp2 and rcp."""
    rng = np.random.default_rng(5)
    v = _silu_inputs()
    want = R.act_ref(v, R.ACT_SILU)
    with np.errstate(over="ignore", under="ignore"):
        e = _within_one_ulp(np.exp(-v.astype(np.float64)), rng)                  # expf within 1 ulp
        got32 = (v / (F32(1) + e).astype(F32)).astype(F32)                       # IEEE division
    for prec, got in (("fp32", got32), ("fp16x3", x3_silu_model(v, rng, True))):
        A = CR.act_slack(v.astype(np.float64), prec, R.ACT_SILU)
        err = np.abs(got.astype(np.float64) - want)
        nz = A > 0
        print("SiLU %s: worst |err| / A %.3f" % (prec, (err[nz] / A[nz]).max()))
        assert (err <= A).all() and (err[nz] / A[nz]).max() > 0.2
    for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY):
        assert not CR.act_slack(v.astype(np.float64), "fp16", act).any()


def test_x3_dropped_term_covers_the_three_product_form():
    """sum over k of (a_hi w_hi + 2^-11 (a_hi w_lo + a_lo w_hi)) in float64 against the full product of the joined values: the difference
    is inside x3_dropped, on normal operands within 1.002 * 2^-22 S and on half-subnormal ones (where it is 2^-11 of the product) too."""
    rng = np.random.default_rng(6)
    for xs, wsc in ((1.0, 1.0), (3e-5, 1.0), (1.0, 2e-5), (40.0, 0.3)):
        x, w = rng.standard_normal((2, 16, 6, 7)) * xs, rng.standard_normal((8, 16, 3, 3)) * wsc
        if xs >= 1 and wsc >= 0.3:       # normal hi halves only: no value below 2^-10
            x, w = np.where(np.abs(x) < 2.0 ** -10, 2.0 ** -10, x), np.where(np.abs(w) < 2.0 ** -10, 2.0 ** -10, w)
        x, w = R.storage_round(x.astype(F32), "fp16x3"), R.storage_round(w.astype(F32), "fp16x3")
        xh, xl = [a.astype(np.float64) for a in R.x3_split(x)]
        wh, wl = [a.astype(np.float64) for a in R.x3_split(w)]
        assert np.array_equal(xh + xl / 2048, x.astype(np.float64)) and np.array_equal(wh + wl / 2048, w.astype(np.float64))   # the split of a stored pair is the pair
        three = CR._conv64(xh, wh, None, 1, 1) + (CR._conv64(xh, wl, None, 1, 1) + CR._conv64(xl, wh, None, 1, 1)) / 2048
        full = CR._conv64(x, w, None, 1, 1)
        D = CR.x3_dropped(x, w, 1, 1)
        S = CR._conv64(np.abs(x), np.abs(w), None, 1, 1)
        assert (np.abs(three - full) <= D + 1e-15 * S).all()
        if xs >= 1 and wsc >= 0.3:
            assert (D <= 1.002 * 2.0 ** -22 * S).all() and (D >= 0.2 * 2.0 ** -22 * S).mean() > 0.5


# ------------------------------------------------------------------------------------------------------------------------- mutations
MUT_PRECS = list(R.PRECISIONS)
CIN, COUT, HW = 40, 80, (80, 112)     # a ragged layer: 40 -> 80 channels (five 8-channel groups in, no multiple of 32 either side)
QUIET = 37                            # an output channel with weights 1/50 of the others (a class-branch channel before training has such)
CH = slice(32, 48)                    # the 16 output channels of one MFMA tile; with 16 pixels of a row: what one wave computes


def _base(prec):
    """The layer the mutations are applied to: silu(conv3x3(x) + b) + r on 3 frames, frames 1 and 2 neighbours in a video (0.8 % apart), a
    residual a tenth of the activations.  Returns the operands, the float64 reference and the correct result as `prec` stores it."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3, CIN) + HW)
    x[2] = x[1] + 0.008 * rng.standard_normal((CIN,) + HW)
    x = R.storage_round(x.astype(F32), prec)
    w = rng.standard_normal((COUT, CIN, 3, 3)) * np.sqrt(2.0 / (CIN * 9))
    w[QUIET] *= 0.02
    w = CR.weights_as_stored(w.astype(F32), prec)
    b = (rng.standard_normal(COUT) * 0.05).astype(F32)
    r = 0.1 * rng.standard_normal((3, COUT) + HW)
    r[2] = r[1] + 0.0008 * rng.standard_normal((COUT,) + HW)       # (the residual is a feature map of the same frames)
    r = R.storage_round(r.astype(F32), prec)
    want, S, v = CR.conv_layer_ref(x, w, b, 1, 1, R.ACT_SILU, r, CR.RES_AFTER_ACT)
    slack = CR.conv_slack(x, w, 1, 1, R.ACT_SILU, prec, S, v)
    good = R.storage_round(want.astype(F32), prec)
    return dict(x=x, w=w, b=b, r=r, want=want, S=S, v=v, slack=slack, good=good)


_BASE = {}


def base(prec):
    if prec not in _BASE:
        _BASE[prec] = _base(prec)
    return _BASE[prec]


def _redo(B, prec, frame, x=None, w=None, res_mode=CR.RES_AFTER_ACT):
    """Frame `frame` of the layer recomputed in float64 with a changed operand, stored in `prec`; the other frames are the correct ones."""
    f = slice(frame, frame + 1)
    v = CR._conv64((B["x"] if x is None else x)[f], B["w"] if w is None else w, B["b"], 1, 1)
    want = R.act_ref(v, R.ACT_SILU) + B["r"][f] if res_mode == CR.RES_AFTER_ACT else R.act_ref(v + B["r"][f], R.ACT_SILU)
    m = B["good"].copy()
    m[f] = R.storage_round(want.astype(F32), prec)
    return m


def _region(B, *index):
    region = np.zeros(B["good"].shape, bool)
    region[index] = True
    return region


def mut_corner_tap(B, prec):
    """Frame 0, output pixel (0, 0), one MFMA tile's 16 output channels: the tap (2, 2) -- input pixel (1, 1), inside the image -- is dropped."""
    x = B["x"].copy()
    x[0, :, 1, 1] = 0                                   # (of output (0, 0), only the tap (2, 2) reads the changed pixel)
    return _redo(B, prec, 0, x=x), _region(B, 0, CH, 0, 0)


def mut_tile_seam(B, prec):
    """Frame 1, a tile of 8 rows ending at column 31: its last column is computed as if the input ended there (column 32 read as padding)."""
    x = B["x"].copy()
    x[1, :, :, 32] = 0
    return _redo(B, prec, 1, x=x), _region(B, 1, CH, slice(8, 16), 31)


def mut_ragged_group(B, prec):
    """Frame 2, one MFMA tile (16 pixels of a row x 16 channels): the last 8-channel group of the 40 input channels (32..39) is read from
    the group before (24..31)."""
    x = B["x"].copy()
    x[:, 32:40] = x[:, 24:32]
    return _redo(B, prec, 2, x=x), _region(B, 2, CH, 5, slice(16, 32))


def mut_transposed_taps(B, prec):
    """The kh and kw taps transposed on one (quiet) output channel, everywhere in frame 1."""
    w = B["w"].copy()
    w[QUIET] = w[QUIET].transpose(0, 2, 1)
    return _redo(B, prec, 1, w=w), _region(B, 1, QUIET)


def mut_frames_swapped(B, prec):
    """Frames 1 and 2 swapped on one MFMA tile."""
    m = B["good"].copy()
    m[1, CH, 20, 32:48], m[2, CH, 20, 32:48] = B["good"][2, CH, 20, 32:48], B["good"][1, CH, 20, 32:48]
    return m, _region(B, slice(1, 3), CH, 20, slice(32, 48))


def mut_residual_order(B, prec):
    """One MFMA tile of frame 0: silu(conv + b + r) where the layer says silu(conv + b) + r."""
    return _redo(B, prec, 0, res_mode=CR.RES_BEFORE_ACT), _region(B, 0, CH, 17, slice(48, 64))


def mut_two_ulp(B, prec):
    """One element stored 2 ulps of the storage type off (the element whose value is largest against its S: the slack is smallest there)."""
    g = B["good"]
    i = np.unravel_index(np.argmax(np.abs(B["want"]) / B["S"]), g.shape)
    m = g.copy()
    u = {"fp16": R.ulp16, "bf16": R.ulpbf}[prec](B["want"][i])
    m[i] = F32(g[i] + 2 * u)
    return m, _region(B, *i)


# (the seam and the ragged group, 128 and 256 elements of 2.2 M, leave a rel-L2 of 4e-3 and 7e-3: under bf16's 1e-2, above fp16's 1.5e-3 --
# the norm's blindness to THEM is asserted in bf16 only; fp32's and fp16x3's max|d| criteria see every mutation but none is local)
# name -> (mutation, precisions it applies to, precisions in which the whole-tensor criterion is asserted to let it through)
MUTATIONS = {
    "corner_tap": (mut_corner_tap, MUT_PRECS, ("bf16", "fp16")),
    "tile_seam": (mut_tile_seam, MUT_PRECS, ("bf16",)),
    "ragged_group": (mut_ragged_group, MUT_PRECS, ("bf16",)),
    "transposed_taps": (mut_transposed_taps, MUT_PRECS, ("bf16", "fp16")),
    "frames_swapped": (mut_frames_swapped, MUT_PRECS, ("bf16", "fp16")),
    "residual_order": (mut_residual_order, MUT_PRECS, ("bf16", "fp16")),
    "two_ulp": (mut_two_ulp, ("fp16", "bf16"), ("bf16", "fp16")),
}


@pytest.mark.parametrize("name,prec", [(n, p) for n in MUTATIONS for p in MUTATIONS[n][1]])
def test_checker_rejects_what_the_norm_lets_through(name, prec):
    """A float64-correct result stored through storage_round, one local mistake applied inside `region`: the checker accepts the correct
    tensor, rejects the mutated one, and puts every rejection inside the region; the whole-tensor criterion this file's GPU sibling
    replaces (rel-L2 of the mutated tensor against the correct one at the old tolerance) PASSES on the same tensor."""
    fn, precs, norm_blind = MUTATIONS[name]
    B = base(prec)
    ok0, w0, _ = CR.check(B["good"], B["want"], prec, B["slack"])
    assert ok0.all() and w0 <= 1.0
    m, region = fn(B, prec)
    mutated = np.where(region, m, B["good"])
    assert (mutated != B["good"]).any() and not (mutated != B["good"])[~region].any()
    ok, w, err = CR.check(mutated, B["want"], prec, B["slack"])
    old_pass, rel, mx = CR.old_criterion(mutated, B["good"], prec)
    print("%s %s: %d of %d elements changed, checker rejects %d (worst |err| / bound %.1f); rel-L2 %.2e max|d| %.2e -> old criterion %s"
          % (name, prec, int((mutated != B["good"]).sum()), mutated.size, int((~ok).sum()), w, rel, mx, "passes" if old_pass else "fails"))
    assert not ok.all() and w > 1.0, "the checker must reject the mutation"
    assert ok[~region].all(), "and blame nothing outside it"
    if name != "two_ulp":
        assert (~ok[region]).mean() > 0.5, "most of the mutated elements are individually out of bound"
    if prec in norm_blind:
        assert old_pass, "the whole-tensor criterion lets this mutation through: rel-L2 %.2e" % rel


# ------------------------------------------------------------------------------------------------------------------------- accepted stores
@pytest.mark.parametrize("prec", R.PRECISIONS)
@pytest.mark.parametrize("act,rm,f32_out", [(R.ACT_NONE, CR.RES_NONE, False), (R.ACT_SILU, CR.RES_AFTER_ACT, False), (R.ACT_RELU, CR.RES_BEFORE_ACT, False),
                                            (R.ACT_LEAKY, CR.RES_NONE, True)])
def test_checker_accepts_the_correctly_rounded_store(prec, act, rm, f32_out):
    """float32(want64) rounded into the output's storage type (float32 itself for a float32 output) is inside the bound everywhere."""
    L = _layer(np.random.default_rng(8), prec, 24, 16, 3, 1, (9, 11), act, rm)
    want, S, v = CR.conv_layer_ref(*L)
    slack = CR.conv_slack(L[0], L[1], L[3], L[4], act, prec, S, v)
    got = R.storage_round(want.astype(F32), CR.out_prec(prec, f32_out))
    ok, w, err = CR.check(got, want, prec, slack, f32_out)
    assert ok.all() and w <= 1.0
    if f32_out and prec != "fp32":      # a float32 output gets no store term: the 16-bit rounding of the same values is out of bound
        ok16, _, _ = CR.check(R.storage_round(want.astype(F32), prec), want, prec, slack, f32_out)
        assert prec == "fp16x3" or (~ok16).mean() > 0.5


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_checker_accepts_a_tie_rounded_either_way(prec):
    """A reference exactly half way between two neighbours of the storage type: both are accepted with NO slack, the next ones are not."""
    lo = R.storage_round(np.random.default_rng(9).uniform(-8, 8, 20000).astype(F32), prec).astype(np.float64)
    u = (R.ulp16 if prec == "fp16" else R.ulpbf)(lo * (1 + 2.0 ** -12))
    up = lo + np.sign(lo) * u
    keep = (lo != 0) & (R._floor_log2(lo) == R._floor_log2(up))     # both neighbours in one binade
    lo, up, u = lo[keep], up[keep], u[keep]
    tie = (lo + up) / 2
    for g in (lo, up):
        assert R.round_ok(g, tie, prec, 0.0).all()
    assert not R.round_ok(lo - np.sign(lo) * u, tie, prec, 0.0).any() and not R.round_ok(up + np.sign(lo) * u, tie, prec, 0.0).any()


def test_nan_and_inf_are_rejected():
    want = np.ones((1, 2, 2, 2))
    got = want.copy().astype(F32)
    got[0, 1, 1, 0] = np.nan
    got[0, 0, 0, 1] = np.inf
    ok, w, err = CR.check(got, want, "bf16", np.full(want.shape, 1e30))
    assert (~ok).sum() == 2
