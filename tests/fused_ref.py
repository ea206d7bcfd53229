"""Float64 reference and per-element bound of a FUSED conv launch (csrc/conv_pair.hip, conv_c2f*.hip, the stems with a second conv or a
max-pool behind them, conv_halo8.hip with a folded projection), built on tests/conv_ref.py.  No GPU and no project code in here: torch /
NumPy only, tested by tests/test_fused_ref_cpu.py, used by tests/test_gpu_fused_exact.py.

A fused launch keeps the tensor between two convs in LDS, so it cannot be fetched -- but it can be computed: in float64 from the fetched
input, then rounded the way the kernel stores it.  What is left to account for is how the device's rounding of that tensor may differ
from the reference's.

One stage  t = act(conv(x, w) + b [+ r]) | act(conv(x, w) + b) + r  that is STORED (16-bit in LDS; hi / lo planes in fp16x3):
  t64      conv_ref.conv_layer_ref on the stage's reference operands;  slack1 = conv_ref.conv_slack (+ the chained term of its own input),
  t_ref    t64 rounded into the storage type, from float64 directly (round64: one rounding, ties to even),
  t_dev    what the device holds: round(t64 + e), |e| <= slack1 by the single-layer bound.
16-bit types.  Rounding is monotone, so t_dev = t_ref unless a rounding boundary (the midpoint between two neighbours of the storage type)
lies within slack1' = slack1 + 2^-24 |t64| of t64 (the device rounds a float32, which is itself a rounding of its exact value): evaluated
as  round64(t64 - slack1') != round64(t64 + slack1').  Such an element is AMBIGUOUS and
    |t_dev - t_ref| <= |t_dev - (t64 + e)| + |e| + |t64 - t_ref| <= ulp(|t64| + slack1') / 2 + slack1' + ulp(t64) / 2
                    <= delta1 = slack1' + ulp(|t64| + slack1');
for every other element delta1 = 0.  (delta1 is slack1' + ulp, not ulp: near zero the fp16 spacing is below the slack and a flip can span
several ulps.)  Split precision: the spacing is below the slack everywhere, every element takes
    delta1 = slack1 + 2 R_x3(|t64| + slack1)            (one split of the device's value, one of the reference's, the slack between them).

The next stage is evaluated on t_ref, with the single-layer bound and the chained term:
    |got - want| <= R(want) + slack2 + L conv(delta1, |w2|)      [+ delta_r of a residual behind the activation, unscaled]
L bounds the activation's slope: 1 for none, ReLU and leaky ReLU.  SiLU: s(v) = v sig(v), s'(v) = sig (1 + v (1 - sig)),
s''(v) = sig (1 - sig) (2 + v (1 - 2 sig)) = 0  <=>  v tanh(v / 2) = 2  <=>  v = +-2.39936; s'(2.39936) = 0.916755 * (1 + 2.39936 * 0.083245)
= 1.09984 and s'(-2.39936) = -0.09984; s' -> 1 and 0 at +-inf, so |s'| <= 1.0998 < L = 1.1.  The chained term also moves the magnitudes S
the stage's own slack is taken on, by at most itself: it enters multiplied by (1 + 2^-18) (K_CONV 2^-24 < 2^-19, the activation term is
smaller still).  Stages compose -- a C2f block is four applications (cv1, conv A, conv B + y1, cv2 over the concat) -- and a stage whose
input carries a delta has it in its own slack1, so its ambiguity test widens by L conv(delta_in, |w|).  No element is exempted anywhere:
an ambiguous element only widens the bound of the elements that read it.

PROBE stages.  A later stage whose weights are a signed selection (each output channel +-1 on one (tap, channel), bias 0: exact in every
storage type, every other product an exact zero) makes the earlier stage visible element by element: it is then evaluated on t64 itself
with the DIRECT bound |t_dev - t64| <= R(t64) + slack1 as its input's delta, and with no accumulation term of its own (`exact=True`):
    |got - act(+-t64)| <= R(want) + L (R(t64) + slack1) + A        (+ one fp32 rounding of the sum where a residual is added, and one of
                                                                     the joined pair in the split precision).

Fused max-pool (stem + pool): rounding is monotone and so is the maximum, so got lies in [maxpool(want - b), maxpool(want + b)],
b = R(want) + slack of the conv's elements, -inf padding (pool_interval).

Folded projection (conv_h8 + shortcut): no stage is stored; one expression act(conv3x3(t) + b + conv1x1_s2(x) + b_d) accumulated in fp32,
S = the sum of both magnitude sums (folded_ref).

Figures of tests/test_fused_ref_cpu.py (CPU, reference and float32 emulation only; 23 x 37 maps, 3 frames, inputs +-2, He weights):
  3x3 -> 3x3 SiLU pair with shortcut, 16 | 32 channels:  ambiguous share of the intermediate fp16 29.8 | 37.8 %, bf16 5.4 | 7.1 %;  median chained
      term / R(want) fp16 1.96 | 3.63, bf16 0.19 | 0.42 (asserted <= 4 and <= 1; the naive form conv(R(t) + slack1, |w2|) gives 8.5 - 12.3);
      intermediate elements the emulation rounds the other way 0.09 - 0.12 % (fp16), 0.007 - 0.011 % (bf16), none outside the ambiguous set
  C2f(32, n = 1, shortcut), four stages:  ambiguous share of cv1 | conv A | conv B  fp16 16.8 | 92.1 | 100 %, bf16 2.9 | 41.2 | 96.6 %;  median
      chained term / R(want) of conv A | conv B | cv2  fp16 3.06 | 47.2 | 254, bf16 0.24 | 6.67 | 48.9, fp16x3 2400 | 21699 | 102648 (R_x3 is
      2^-22 |want|; the term is the K_CONV 2^-24 S slack of the stages before).  A worst-case term grows by about sum |w| per stage, and once
      it passes a spacing every element behind it is ambiguous: from conv B on the chain holds the block's structure (the mutations) but no
      longer a rounding -- that is what the probe stages are for (test_c2f_chain_figures holds these figures)
  emulation's worst |err| / bound, every ambiguous element forced either way: 0.70 - 0.998 in the 16-bit types, 0.26 - 0.67 in fp16x3.
On the device (tests/test_gpu_fused_exact.py, frames +-1 behind a 1x1 expand): pair ambiguous 22 - 31 % (fp16), 4 - 6 % (bf16), chained term
median 1.8 - 9.8 R(want) (fp16), 0.17 - 1.04 (bf16); worst |err| / bound 0.64 - 0.91 (fp16), 0.97 - 0.995 (bf16); probe cases 0.94 - 0.98."""
import numpy as np

import conv_ref as CR
import ops_ref as R
from conv_ref import RES_NONE, RES_AFTER_ACT, RES_BEFORE_ACT
from ops_ref import ACT_NONE, ACT_SILU, ACT_RELU, ACT_LEAKY, EPS32

SILU_SLOPE = 1.1          # > 1.09984, derived above
CHAIN_S = 1 + 2.0 ** -18  # the chained term's own share of the stage's slack


def slope(act):
    assert act in (ACT_NONE, ACT_SILU, ACT_RELU, ACT_LEAKY), act
    return SILU_SLOPE if act == ACT_SILU else 1.0


def _ulp(v, prec):
    return R.ulp16(v) if prec == "fp16" else R.ulpbf(v)


def round64(t, prec):
    """A float64 array rounded ONCE into the storage type (ties to even), returned as float64.  16-bit: rint(t / ulp) * ulp (a result that
    reaches the next binade is that binade's first value: still exact).  fp16x3: elem16.h's x3_split on the float64 value -- hi = half(t),
    zero below 2^-14; lo = half((t - hi) 2^11) -- joined exactly (hi + 2^-11 lo is what the MFMAs read)."""
    t = np.asarray(t, np.float64)
    if prec in ("fp16", "bf16"):
        u = _ulp(t, prec)
        return np.rint(t / u) * u
    if prec == "fp16x3":
        hi = np.where(np.abs(t) >= 2.0 ** -14, round64(t, "fp16"), 0.0)
        return hi + round64((t - hi) * 2048.0, "fp16") / 2048.0
    raise ValueError(prec)


def conv_abs(d, w, stride, pad):
    """conv(d, |w|) in float64: how far a per-element bound d on the input moves the pre-activation sum."""
    return CR._conv64(np.asarray(d, np.float64), np.abs(np.asarray(w, np.float64)), None, stride, pad)


class Stage:
    """One evaluated stage.  want, S, v: conv_ref.conv_layer_ref;  chain: L conv(dx, |w|) [+ the residual's delta];  slack: conv_slack plus
    the chained term -- |device value before its store - want| <= slack;  yard: the stage's yardstick ratios (worst, torch, sequential)."""

    def __init__(self, prec, want, S, v, slack, chain, yard):
        self.prec, self.want, self.S, self.v, self.slack, self.chain, self.yard = prec, want, S, v, slack, chain, yard

    def bound(self, f32_out=False):
        """R(want) + slack: the bound of the stage's output as the launch writes it."""
        return R.store_bound(self.want, CR.out_prec(self.prec, f32_out)) + self.slack

    def check(self, got, f32_out=False):
        """(ok per element, worst |err| / bound, worst |err|)."""
        return CR.check(got, self.want, self.prec, self.slack, f32_out)

    def stored(self):
        """(t_ref, delta1, ambiguous): the stage as the NEXT stage's reference operand -- the ambiguity form of the module docstring."""
        t, prec = self.want, self.prec
        ref = round64(t, prec)
        if prec == "fp16x3":
            return ref, self.slack + 2 * R.store_bound(np.abs(t) + self.slack, prec), np.ones(t.shape, bool)
        assert prec in ("fp16", "bf16"), prec
        s1 = self.slack + EPS32 * np.abs(t)
        amb = round64(np.nextafter(t - s1, -np.inf), prec) != round64(np.nextafter(t + s1, np.inf), prec)
        return ref, np.where(amb, s1 + _ulp(np.abs(t) + s1, prec), 0.0), amb

    def direct(self):
        """(t64, R(t64) + slack1): the stage as a PROBE stage's operand."""
        return self.want, R.store_bound(self.want, self.prec) + self.slack


def stage(x, w, b, stride, pad, act, prec, r=None, res_mode=RES_NONE, dx=None, dr=None, exact=False, yard=True):
    """One stage on its reference operands.  x (r): the operand (residual) the reference reads, dx (dr): a per-element bound on how far
    the device's operand is from it (None: it IS the device's, a fetched tensor).  exact: a probe stage (signed selection, bias 0) -- no
    accumulation term, only the activation's."""
    want, S, v = CR.conv_layer_ref(x, w, b, stride, pad, act, r, res_mode)
    if exact:
        wa = np.abs(np.asarray(w, np.float64)).reshape(len(w), -1)
        assert ((wa == 0) | (wa == 1)).all() and (wa.sum(1) == 1).all() and not np.asarray(b).any(), "a probe stage is a signed selection"
        # one product by +-1 and exact zeros: what is left in front of the store is the activation, the fp32 add of a residual, and in the
        # split precision the fp32 join of the selected pair (main + 2^-11 cross: one rounding)
        slack = CR.act_slack(v, prec, act) + ((r is not None) + (prec == "fp16x3")) * EPS32 * S
    else:
        slack = CR.conv_slack(x, w, stride, pad, act, prec, S, v)
    L = slope(act)
    pre = 0.0 if dx is None else conv_abs(dx, w, stride, pad)
    if dr is not None and res_mode == RES_BEFORE_ACT:
        pre = pre + dr
    chain = L * pre + (dr if dr is not None and res_mode == RES_AFTER_ACT else 0.0)
    chain = np.broadcast_to(np.asarray(chain, np.float64), want.shape)
    y = CR.conv_yardstick(x, w, b, stride, pad, act, r, res_mode, want, S) if yard and not exact else (0.0, 0.0, 0.0)
    return Stage(prec, want, S, v, slack + CHAIN_S * chain, chain, y)


# ------------------------------------------------------------------------------------------------------------------------- the fused forms
def pair_ref(x, wa, ba, wb, bb, prec, shortcut, probe=False, yard=True):
    """conv_pair: y = SiLU(B(SiLU(A x))) [+ x].  Returns (stage A, stage B); probe: B is a signed selection, read off A's direct form."""
    A = stage(x, wa, ba, 1, 1, ACT_SILU, prec, yard=yard)
    t, dt = A.direct() if probe else A.stored()[:2]
    r, rm = (x, RES_AFTER_ACT) if shortcut else (None, RES_NONE)
    return A, stage(t, wb, bb, 1, 1, ACT_SILU, prec, r, rm, dx=dt, exact=probe, yard=yard)


def c2f_ref(x, w, b, prec, probe=(), yard=True):
    """conv_c2f16: (y0, y1) = split(SiLU(cv1 x));  t = SiLU(A y1);  y2 = SiLU(B t) + y1;  out = SiLU(cv2 cat(y0, y1, y2)).  w, b: the four
    layers' (cv1, A, B, cv2).  probe: the layers among "cv1", "B", "cv2" that are signed selections -- B and cv2 then read the stage before
    them in its direct form; a cv1 that is a selection leaves the Bottleneck an input with (almost) no ambiguity, so conv A and conv B
    are seen as sharply as a bare pair's.  Returns the four stages (cv1, A, B, cv2)."""
    assert set(probe) <= {"cv1", "B", "cv2"}, probe
    p1, pb, p2 = "cv1" in probe, "B" in probe, "cv2" in probe
    s1 = stage(x, w[0], b[0], 1, 0, ACT_SILU, prec, exact=p1, yard=yard)
    y, dy, _ = s1.stored()
    y1, dy1 = y[:, 16:32], dy[:, 16:32]
    sA = stage(y1, w[1], b[1], 1, 1, ACT_SILU, prec, dx=dy1, yard=yard)
    t, dt = sA.direct() if pb else sA.stored()[:2]
    sB = stage(t, w[2], b[2], 1, 1, ACT_SILU, prec, y1, RES_AFTER_ACT, dx=dt, dr=dy1, exact=pb, yard=yard)
    if p2:
        (y01, d01), (y2, d2) = s1.direct(), sB.direct()
    else:
        y01, d01 = y, dy
        y2, d2 = sB.stored()[:2]
    s2 = stage(np.concatenate([y01, y2], 1), w[3], b[3], 1, 0, ACT_SILU, prec, dx=np.concatenate([d01, d2], 1), exact=p2, yard=yard)
    return s1, sA, sB, s2


def stem2_ref(x, w1, b1, pad1, w2, b2, prec, probe=False, yard=True):
    """stem + second conv: SiLU(conv3x3 s2 p1 (SiLU(conv k x k s2 (x)))).  x: the frame as the stem stores it (storage_round)."""
    s1 = stage(x, w1, b1, 2, pad1, ACT_SILU, prec, yard=yard)
    t, dt = s1.direct() if probe else s1.stored()[:2]
    return s1, stage(t, w2, b2, 2, 1, ACT_SILU, prec, dx=dt, exact=probe, yard=yard)


def pool_interval(st, k=3, s=2, p=1):
    """[maxpool(want - b), maxpool(want + b)] of a stage's output behind a fused max-pool (-inf padding), b = R(want) + slack."""
    b = st.bound()
    return R.maxpool_ref(st.want - b, k, s, p), R.maxpool_ref(st.want + b, k, s, p)


def pool_check(got, lo, hi):
    """(ok per element, worst excursion outside the interval in units of its half width -- 0 inside)."""
    g = np.asarray(got, np.float64)
    ok = np.isfinite(g) & (g >= lo) & (g <= hi)
    half = (hi - lo) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(ok, 0.0, np.maximum(lo - g, g - hi) / half)
    return ok, float(np.nanmax(out)) if out.size else 0.0


def folded_ref(t, w, b, x, wd, bd, act, prec, yard=True):
    """conv_h8 + shortcut: act(conv3x3(t) + b + conv1x1_s2(x) + b_d), both sums in one fp32 accumulator; t and x are fetched tensors.
    The yardstick restates it as the 3x3's two float32 accumulations with the float32 projection added in front of the activation."""
    v3, S3 = CR.conv_sums64(t, w, 1, 1)
    v1, S1 = CR.conv_sums64(x, wd, 2, 0)
    b64, bd64 = np.asarray(b, np.float64)[None, :, None, None], np.asarray(bd, np.float64)[None, :, None, None]
    v = v3 + b64 + v1 + bd64
    S = S3 + np.abs(b64) + S1 + np.abs(bd64)
    want = R.act_ref(v, act)
    slack = CR.K_CONV * EPS32 * S + CR.act_slack(v, prec, act)
    y = (0.0, 0.0, 0.0)
    if yard:
        r32 = (CR.acc_f32_torch(x, wd, 2, 0) + np.asarray(bd, np.float32)[None, :, None, None]).astype(np.float32)
        y = CR.yardstick_from_accs(CR.conv_accs_f32(t, w, 1, 1, want.shape), b, act, r32, RES_BEFORE_ACT, want, S)
    return Stage(prec, want, S, v, slack, np.zeros_like(want), y)


# ------------------------------------------------------------------------------------------------------------------------- probe weights
def selection(cout, cin, k, taps_channels, signs=None):
    """OIHW weights of a signed selection: output channel o reads (tap, channel) = taps_channels[o] with weight signs[o] (default
    alternating +1, -1), everything else zero."""
    w = np.zeros((cout, cin, k, k), np.float32)
    for o, (tap, ch) in enumerate(taps_channels):
        w[o, ch, tap // k, tap % k] = (1.0 if o % 2 == 0 else -1.0) if signs is None else signs[o]
    return w


# ------------------------------------------------------------------------------------------------------------------------- the old criterion
def old_rel_l2(got, ref):
    d = np.asarray(got, np.float64) - np.asarray(ref, np.float64)
    return float(np.linalg.norm(d) / (np.linalg.norm(ref) + 1e-30))


OLD_TOL = {"pair": {"fp16": 2.5e-3, "bf16": 2e-2}, "c2f": {"fp16": 2.5e-3, "bf16": 2e-2, "fp16x3": 3e-6}, "stem2": {"fp16": 1e-2, "bf16": 1e-2, "fp16x3": 3e-6},
           "pool": {"fp16": 1e-2, "bf16": 1e-2}, "folded": {"fp16": 2e-3, "bf16": 1e-2}}     # tests/test_gpu_conv.py, test_gpu_x3.py
