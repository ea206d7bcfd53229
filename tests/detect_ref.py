"""Float64 reference and per-element bound of the v8-layout Detect head (csrc/aux_kernels.hip: detect_v8_kernel, detect_v8_fused_kernel,
detect_v8_fused_x3_kernel), built on tests/conv_ref.py.  No GPU and no project code in here: torch / NumPy only, tested by
tests/test_detect_ref_cpu.py, used by tests/test_gpu_detect_exact.py.

The head.  Per pyramid level two 1x1 convs without activation give 64 box logits (4 sides x 16 DFL bins) and nc class logits per cell;
the decode turns a cell into one column of the (4 + nc, A) head, rows ordered (level, y, x) like the oracle's (oracle/nets.py):
    dist_side = sum_k k softmax(z_side)_k,  k = 0 .. 15             anchor point (ax, ay) = (x + 0.5, y + 0.5)
    x1 = ax - dist_0, y1 = ay - dist_1, x2 = ax + dist_2, y2 = ay + dist_3
    rows 0..3 = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1) * stride          rows 4.. = sigmoid(class logits)
Operands: the hidden maps the two convs read (fetched; exact values of the storage type) with the weights as stored
(conv_ref.weights_as_stored) for the fused kernels; the fetched float32 logits for detect_v8_kernel.

The bound of an element is |got - want| <= bound, want the expression above in float64.  No tolerance is picked: every term is
derived here, U = 2^-24 (one float32 rounding, relative), and the whole bound is multiplied by MARGIN = 1 + 2^-10 for the products of
two rounding terms that the sums below leave out (each below 2^-20 of the term it belongs to in the asserted ranges).

  logit slack dz      conv_ref.conv_slack of the 1x1 conv: K_CONV 2^-24 S plus the split precision's dropped product term, K_CONV as
                      recorded in conv_ref.py; R = 0 (the logit is never stored in 16 bits); zero for a fetched float32 logit.

  sigmoid             p = 1 / (1 + exp(-z)).  The logit's slack moves p by at most p (1 - p) dz e^(2 dz): the derivative is p (1 - p) and
                      each factor changes by at most e^|d| over a step d.  The form's own error, relative on p:
      exact form  (detect_v8_kernel, detect_v8_fused_x3_kernel: 1.0f / (1.0f + expf(-z)), IEEE division)
                      expf within 1 ulp: 2 U on e = exp(-z), which enters d = 1 + e scaled by e / (1 + e) = 1 - p;  fl(1 + e): U;
                      the division: U.   Sum  2 U (1 - p) + 2 U  <= 2^-22.
      fast form   (detect_v8_fused_kernel<Fp16 | Bf16>: fast_rcp(1.0f + __expf(-z)) of elem16.h, __expf(x) = v_exp_f32(x * log2 e))
                      t = fl(-z fl(log2 e)): the constant's and the product's rounding, 2 U |t| absolute, which exp2 turns into a
                      relative error of 2 U |t| ln 2 = 2 U |z| on e;  v_exp_f32 1 ulp: 2 U;  both scaled by 1 - p;  fl(1 + e): U;
                      v_rcp_f32 1 ulp: 2 U.   Sum  2 U (|z| + 1) (1 - p) + 3 U.
      Valid while exp(-z) is a finite normal float32 and no step flushes: |z| + dz <= SIG_Z_MAX = 80, asserted per call.

  DFL                 With m the largest of the side's 16 computed logits the kernels form e_k = exp(fl(z_k - m)), se = sum e_k,
                      sw = sum k e_k, dist = sw / se.  A relative error eps_k of e_k acts on dist exactly like a logit error
                      log(1 + eps_k), and m cancels, so with d_k = dz_k + eta_k
                          |dist' - dist| = |sum (k - dist) s_k (e^(delta_k) - 1)| / sum s_j e^(delta_j)  <=  e^(2 D) sum_k s_k |k - dist| d_k,
                      D = max_k d_k: the first-order sum times the stated margin e^(2 D), which holds for every D; D <= DZ_MAX = 2^-4 is
                      asserted per call so that the margin stays below 1.14 and a case whose logits are that loose is noticed.
                      eta_k, the exponential's relative error:
      exact form      fl(z_k - m): U |z_k - m| absolute on the argument = relative on e_k;  expf 1 ulp: 2 U.     eta = U |z - m| + 2 U
      fast form       the same subtraction;  t = fl(x fl(log2 e)): 2 U |x|;  v_exp_f32 1 ulp: 2 U.               eta = 3 U |z - m| + 2 U
                      The float32 sums: all terms are positive, so 15 adds leave at most 15 U se on se, the 16 products and 15 adds at
                      most 16 U sw on sw, the division U (IEEE) -- 32 U dist, taken as SUMS = 34 U dist (the second order of 1 / (1 - 15 U)
                      included).  An exponential below 2^-126 may come back as zero (v_exp_f32 returns no subnormal) or as a subnormal with
                      fewer bits: at most 2^-126 absolute on e_k against se >= 1 (the largest term is exp(0)), 16 bins, |k - dist| <= 15:
                      FLUSH = 2^-117 grid units, an absolute term.

  box arithmetic      ax, ay are exact.  x1 = fl(ax - dist_0) and x2 = fl(ax + dist_2) carry the distance errors and one rounding each;
                      fl(x1 + x2) one more; the division by 2 is exact; the product with the stride one (exact for 8, 16, 32, counted
                      for any stride):
                          |d cx| <= (stride / 2) (dd_0 + dd_2 + U (|x1| + |x2| + |x1 + x2|)) + U |cx|
                          |d w|  <=  stride      (dd_0 + dd_2 + U (|x1| + |x2| + |x2 - x1|)) + U |w|          (cy, h likewise)

Hardware figures nobody has measured here: "v_exp_f32 and v_rcp_f32 return within 1 ulp" and "expf returns within 1 ulp" are taken over
from conv_ref.py's SiLU derivation (which takes them from the ISA's and the device library's stated accuracy); the terms 2 U for the
exponentials and 2 U for the reciprocal above rest on them.  That v_exp_f32 returns zero instead of a subnormal is the ISA's statement
too; FLUSH covers either behaviour.

The yardstick.  decode_f32 restates the whole decode in NumPy float32 in both forms, every exp / exp2 and reciprocal result moved to one
of the two float32 neighbours of the exact value at random (+-1 ulp), sums strictly sequential, products and adds rounded separately.
decode_yardstick runs it on float32(logits) and divides its error by the bound at dz = |float32(z) - z|: the restatement must sit inside
the bound.  Worst ratios over tests/test_detect_ref_cpu.py's cases (G1, G2, every width, the x40 stress logits; recorded there too):
box rows 0.328 (exact) / 0.327 (fast), probabilities 0.825 (exact) / 0.739 (fast) -- YARD below, which that test reproduces.  Every GPU
case re-measures the ratio on its own fetched operands (a CPU computation), prints it and asserts that it stays inside the bound: up to
0.389 on the box rows (the fp16 stress case), 0.820 on the probabilities.  No device value enters a bound.

The sink.  SINK = true kernels write per anchor the best probability and its first arg-max instead of the class rows.  sink_ref gives the
float64 best and the classes the bound cannot tell from it; sink_matches_rows is the exact statement against a run that wrote the rows."""
import numpy as np

import conv_ref as CR
from ops_ref import ACT_NONE, EPS32

U = EPS32
F32 = np.float32
MARGIN = 1.0 + 2.0 ** -10
SIG_Z_MAX = 80.0
DZ_MAX = 2.0 ** -4
FLUSH = 2.0 ** -117
SUMS = 34.0
FORMS = ("exact", "fast")
YARD = {"exact": (0.329, 0.826), "fast": (0.328, 0.740)}      # the recorded worst ratios of the restatements (box rows, probability rows)
LOG2E = F32(1.4426950408889634)


def form_of(prec, fused):
    """The sigmoid / softmax form of the kernel that runs the head: the fast form in the 16-bit fused kernel only."""
    return "fast" if fused and prec in ("fp16", "bf16") else "exact"


def _sizes_of(maps):
    return [tuple(m.shape[2:]) for m in maps]


def _flat(a):
    return a.reshape(a.shape[0], a.shape[1], -1)


# ------------------------------------------------------------------------------------------------------------------------- reference
def logits_ref(hidden, w, b, prec):
    """One 1x1 conv without activation in float64 on (B, C, h, w) and its slack dz, both (B, cout, h * w) in (y, x) order."""
    want, S, v = CR.conv_layer_ref(hidden, w, b, 1, 0, ACT_NONE)
    return _flat(want), _flat(CR.conv_slack(hidden, w, 1, 0, ACT_NONE, prec, S, v))


def _level_ref(zb, zc, dzb, dzc, hw, stride, form):
    """One level: (want, bound) of shape (B, 4 + nc, h * w)."""
    B, (h, w) = zb.shape[0], hw
    z = zb.reshape(B, 4, 16, h * w)
    x = z - z.max(2, keepdims=True)
    e = np.exp(x)
    s = e / e.sum(2, keepdims=True)
    k = np.arange(16.0).reshape(1, 1, 16, 1)
    dist = (s * k).sum(2)                                                    # (B, 4, hw)
    eta = (U if form == "exact" else 3 * U) * np.abs(x) + 2 * U
    d = dzb.reshape(B, 4, 16, h * w) + eta
    D = d.max(2)
    assert D.max() <= DZ_MAX, "the DFL bound is stated for logit slacks up to %g, this case has %g" % (DZ_MAX, D.max())
    dd = np.exp(2 * D) * (s * np.abs(k - dist[:, :, None]) * d).sum(2) + SUMS * U * dist + FLUSH
    ax, ay = (np.arange(h * w) % w) + 0.5, (np.arange(h * w) // w) + 0.5
    x1, y1, x2, y2 = ax - dist[:, 0], ay - dist[:, 1], ax + dist[:, 2], ay + dist[:, 3]
    st = float(stride)
    box = np.stack([(x1 + x2) / 2 * st, (y1 + y2) / 2 * st, (x2 - x1) * st, (y2 - y1) * st], 1)
    rx, ry = U * (np.abs(x1) + np.abs(x2)), U * (np.abs(y1) + np.abs(y2))
    bbox = np.stack([st / 2 * (dd[:, 0] + dd[:, 2] + rx + U * np.abs(x1 + x2)), st / 2 * (dd[:, 1] + dd[:, 3] + ry + U * np.abs(y1 + y2)),
                     st * (dd[:, 0] + dd[:, 2] + rx + U * np.abs(x2 - x1)), st * (dd[:, 1] + dd[:, 3] + ry + U * np.abs(y2 - y1))], 1) + U * np.abs(box)
    assert np.abs(zc).max() + dzc.max() <= SIG_Z_MAX, "the sigmoid bound is stated for |z| <= %g, this case has %g" % (SIG_Z_MAX, np.abs(zc).max())
    p = 1.0 / (1.0 + np.exp(-zc))
    q = 1.0 / (1.0 + np.exp(zc))                                             # 1 - p without cancellation
    rel = 2 * U * q + 2 * U if form == "exact" else 2 * U * (np.abs(zc) + 1) * q + 3 * U
    bp = p * q * dzc * np.exp(2 * dzc) + rel * p
    return np.concatenate([box, p], 1), MARGIN * np.concatenate([bbox, bp], 1)


def decode_ref(zb, zc, dzb, dzc, sizes, strides, form):
    """The decode in float64 from per-level logits zb[l] (B, 64, h w), zc[l] (B, nc, h w) with slacks dzb, dzc (arrays, or None for
    logits that ARE the kernel's operands).  Returns (want, bound), each (B, 4 + nc, A)."""
    assert form in FORMS, form
    out = []
    for l in range(len(zb)):
        b64, c64 = np.asarray(zb[l], np.float64), np.asarray(zc[l], np.float64)
        out.append(_level_ref(b64, c64, np.zeros_like(b64) if dzb is None else dzb[l], np.zeros_like(c64) if dzc is None else dzc[l], sizes[l], strides[l], form))
    return np.concatenate([o[0] for o in out], 2), np.concatenate([o[1] for o in out], 2)


def v8_logits_ref(box_logits, cls_logits, strides, form="exact"):
    """The entry for detect_v8_kernel: fetched float32 logits, NCHW per level -- no logit slack."""
    return decode_ref([_flat(z) for z in box_logits], [_flat(z) for z in cls_logits], None, None, _sizes_of(box_logits), strides, form)


def v8_head_ref(hidden_box, hidden_cls, w_box, b_box, w_cls, b_cls, strides, prec, form=None, info=None):
    """The fused head: per level the hidden maps (B, cb | cc, h, w) as fetched, the two 1x1 convs' weights as stored and float32 biases.
    Returns (want, bound), each (B, 4 + nc, A); info (a dict) receives the float64 logits and their slacks."""
    form = form_of(prec, True) if form is None else form
    zb, zc, dzb, dzc = [], [], [], []
    for l in range(3):
        z, dz = logits_ref(hidden_box[l], w_box[l], b_box[l], prec)
        zb.append(z); dzb.append(dz)
        z, dz = logits_ref(hidden_cls[l], w_cls[l], b_cls[l], prec)
        zc.append(z); dzc.append(dz)
    if info is not None:
        info.update(zb=zb, zc=zc, dzb=dzb, dzc=dzc, form=form, max_box_logit=max(float(np.abs(z).max()) for z in zb),
                    max_cls_logit=max(float(np.abs(z).max()) for z in zc), max_dz=max(float(d.max()) for d in dzb + dzc))
    return decode_ref(zb, zc, dzb, dzc, _sizes_of(hidden_box), strides, form)


def check(got, want, bound):
    """(ok per element, worst |err| / bound over the box rows, over the probability rows).  NaN / inf are never ok."""
    g = np.asarray(got, np.float64)
    err = np.abs(g - want)
    ok = np.isfinite(g) & (err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(g), r, np.inf)
    return ok, float(r[:, :4].max()), float(r[:, 4:].max())


# ------------------------------------------------------------------------------------------------------------------------- yardstick
def within_one_ulp(exact64, rng):
    """A float32 result with an error below 1 ulp: one of the two float32 neighbours of the exact value, picked at random per element."""
    with np.errstate(over="ignore", under="ignore"):
        near = np.asarray(exact64, np.float64).astype(F32)
    below = np.where(near.astype(np.float64) > exact64, np.nextafter(near, F32(-np.inf)), near).astype(F32)
    above = np.where(below.astype(np.float64) < exact64, np.nextafter(below, F32(np.inf)), below).astype(F32)
    return np.where(rng.integers(0, 2, near.shape) == 1, above, below).astype(F32)


def _exp_f32(x, form, rng):
    """exp of a float32 array the way the form computes it, the result +-1 ulp; the fast form returns no subnormal."""
    if form == "exact":
        return within_one_ulp(np.exp(x.astype(np.float64)), rng)
    t = (x * LOG2E).astype(F32)
    e = within_one_ulp(np.exp2(t.astype(np.float64)), rng)
    return np.where(e < F32(2.0 ** -126), F32(0), e).astype(F32)


def decode_f32(zb, zc, sizes, strides, form, seed=0, bins=None, use_max=True):
    """The whole decode in NumPy float32 on float32 logits (module docstring: the yardstick).  bins / use_max are the two knobs
    tests/test_detect_ref_cpu.py's wrong kernels need inside the softmax; a kernel has neither."""
    rng = np.random.default_rng(seed)
    one, half = F32(1), F32(0.5)
    kk = np.arange(16, dtype=F32) if bins is None else np.asarray(bins, F32)
    out = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for l in range(len(zb)):
            (h, w), st = sizes[l], F32(strides[l])
            B = zb[l].shape[0]
            z = np.asarray(zb[l], F32).reshape(B, 4, 16, h * w)
            x = (z - z.max(2, keepdims=True)).astype(F32) if use_max else z
            e = _exp_f32(x, form, rng)
            se, sw = np.zeros((B, 4, h * w), F32), np.zeros((B, 4, h * w), F32)
            for k in range(16):
                se = (se + e[:, :, k]).astype(F32)
                sw = (sw + (e[:, :, k] * kk[k]).astype(F32)).astype(F32)
            dist = (sw / se).astype(F32)
            ax, ay = ((np.arange(h * w) % w).astype(F32) + half), ((np.arange(h * w) // w).astype(F32) + half)
            x1, y1, x2, y2 = (ax - dist[:, 0]).astype(F32), (ay - dist[:, 1]).astype(F32), (ax + dist[:, 2]).astype(F32), (ay + dist[:, 3]).astype(F32)
            two = F32(2)
            box = np.stack([((x1 + x2).astype(F32) / two * st), ((y1 + y2).astype(F32) / two * st), ((x2 - x1).astype(F32) * st), ((y2 - y1).astype(F32) * st)], 1).astype(F32)
            c = np.asarray(zc[l], F32)
            d = (one + _exp_f32(-c, form, rng)).astype(F32)
            p = (one / d).astype(F32) if form == "exact" else within_one_ulp(1.0 / d.astype(np.float64), rng)
            out.append(np.concatenate([box, p], 1))
    res = np.concatenate(out, 2)
    assert res.dtype == F32
    return res


def decode_yardstick(zb, zc, sizes, strides, form, seed=0):
    """(worst |f32 - f64| / bound over the box rows, over the probability rows) of decode_f32 on float32(logits), the bound taken at the
    rounding's own dz = |float32(z) - z| (zero for logits that are float32 already)."""
    zb64, zc64 = [np.asarray(z, np.float64) for z in zb], [np.asarray(z, np.float64) for z in zc]
    zb32, zc32 = [z.astype(F32) for z in zb64], [z.astype(F32) for z in zc64]
    want, bound = decode_ref(zb64, zc64, [np.abs(a - b) for a, b in zip(zb32, zb64)], [np.abs(a - b) for a, b in zip(zc32, zc64)], sizes, strides, form)
    _, rb, rp = check(decode_f32(zb32, zc32, sizes, strides, form, seed), want, bound)
    return rb, rp


# ------------------------------------------------------------------------------------------------------------------------- sink
def sink_ref(want_cls, bound_cls):
    """Per anchor of (..., nc, A) class rows: (the float64 best probability, admissible[..., nc, A], ambiguous[..., A]).  A class is
    admissible when its want + bound reaches the largest want - bound; an anchor is ambiguous when more than one class is admissible
    and the admissible classes are not exact float64 ties."""
    lo = (want_cls - bound_cls).max(-2, keepdims=True)
    adm = want_cls + bound_cls >= lo
    w = np.where(adm, want_cls, np.nan)
    tie = np.nanmax(w, -2) == np.nanmin(w, -2)
    return want_cls.max(-2), adm, (adm.sum(-2) > 1) & ~tie


def sink_matches_rows(conf, cls, rows):
    """The sink against the class rows (..., nc, A) of a run without it: conf bit-identical to the maximum, cls its FIRST arg-max."""
    rows = np.asarray(rows, F32)
    return np.array_equal(np.asarray(conf, F32).view(np.uint32), rows.max(-2).view(np.uint32)) and np.array_equal(np.asarray(cls), np.argmax(rows, -2))
