"""Float64 references and per-element bounds of the v5-layout and v6 Detect decodes (csrc/aux_kernels.hip: detect_v5_kernel,
detect_v5_fused_kernel with pack_weights_det5_kernel, detect_v6_kernel, detect_v6_dfl_kernel), next to tests/detect_ref.py (the v8 layout)
and built on it and on tests/conv_ref.py.  No GPU and no project code in here: torch / NumPy only, tested by
tests/test_detect56_ref_cpu.py, used by tests/test_gpu_detect56_exact.py.

Heads are (B, A, no), no = nc + 5, rows contiguous.  No device value enters a reference or a bound; U = 2^-24 is one float32 rounding
(relative), every bound is multiplied by detect_ref.MARGIN = 1 + 2^-10 for the products of two rounding terms the sums leave out.

v5 layout   row = row_off[l] + a hw_l + p (level l, anchor a, cell p = y nx + x; row_off[l] = 3 sum of the earlier levels' cells), built
            here with integer reshapes only.  With s = sigmoid(z) of the row's logit z[l][b, a no + c, p]:
                c = 0  (2 s - 0.5 + x) stride      c = 1  (2 s - 0.5 + y) stride      c = 2, 3  (2 s)^2 anchor[l][a][c - 2]      c >= 4  s
            z: the fetched float32 logits for detect_v5_kernel (exact form, no slack); for detect_v5_fused_kernel (fast form) conv_ref's
            float64 1x1 conv of the fetched 16-bit feature map with the weights as stored and the float32 bias, and its slack dz
            (detect_ref.logits_ref: K_CONV 2^-24 S, K_CONV = 4 x the recorded conv yardstick).
v6          row = row_off[l] + p.  Anchor point (ax, ay) = (x + 0.5, y + 0.5); x1 = ax - d0, y1 = ay - d1, x2 = ax + d2, y2 = ay + d3;
            columns 0..3 = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1) stride; column 4 = 1.0f exactly (bound 0: compared for
            equality); columns 5.. = sigmoid(class logit), exact form.  Without DFL d_k is the fetched float32 reg channel k; with DFL
            d_k = sum_i softmax(z[17 k .. 17 k + 16])_i i over 17 bins.  All logits are fetched float32: no slack.

Bound terms, from the kernels' code
  sigmoid     p = 1 / (1 + exp(-z)), q = 1 - p.  The two forms of detect_ref (its docstring derives them), relative on p:
                  exact  1.0f / (1.0f + expf(-z)), IEEE division          2 U q + 2 U
                  fast   fast_rcp(1.0f + __expf(-z))                      2 U (|z| + 1) q + 3 U
              the logit's slack moves p by at most p q dz e^(2 dz).  detect_ref states them while exp(-z) is a normal float32
              (|z| <= 80); the stress cases here go past that on purpose, so one absolute term is added and the rest re-read:
              SIG_FLUSH = 2^-126.  z > 87: e = exp(-z) is subnormal or flushed to zero -- at most 2^-126 absolute on e, which enters
              d = 1 + e and p with a factor below 1.  z < -87: e is huge, p < 2^-125; the result 1 / d may come back subnormal with fewer
              bits or as zero (v_rcp_f32 returns no subnormal), and an e that rounds past the largest float32 gives p = 0 where the exact
              p is below 2^-127: at most 2^-126 absolute either way.  In between the relative terms hold as derived: they are first-order
              in the relative error of e, at most 2 U (|z| + 1) < 2^-12 for |z| <= SIG56_Z_MAX = 1000 (asserted), whose square MARGIN covers.
              ds := p q dz e^(2 dz) + rel p + SIG_FLUSH is the absolute bound of a probability column.
  v5 x / y    o = fl(fl(fl(2 s - 0.5) + g) stride); 2 s is exact.  t1 = fl(2 s - 0.5): U |t1|;  t2 = fl(t1 + g): U |t2|;  the product: U |o|
              (exact for a power-of-two stride, counted for any).  An fma for the first step rounds once instead -- not more.
                  |d o| <= stride (2 ds + U |2 s - 0.5| + U |2 s - 0.5 + g|) + U |o|
  v5 w / h    t = 2 s exact, dt = 2 ds;  fl(t t): U t^2;  the product with the float32 anchor: U |o|.
              Past z = -43 the square leaves the normal range: fl(t t) and the product may come back subnormal with fewer bits or
              flushed, at most SIG_FLUSH = 2^-126 absolute each (the stress case's restatement shows the term: without it its w / h
              sit 10^6 bounds off at 10^-60).
                  |d o| <= anchor (2 t dt + dt^2 + SIG_FLUSH) + 2 U |o| + SIG_FLUSH
              For the fused kernel ds carries dz through p q, so x / y move by 2 stride p q dz and w / h by 2 (2 s) 2 p q anchor dz
              (the derivative of (2 s)^2 anchor), each times e^(2 dz).
  v6 box      ax, ay exact.  x1 = fl(ax - d0): dd0 + U |x1|;  x2 likewise;  fl(x1 + x2) resp. fl(x2 - x1): U |.|;  the halving exact;
              the product with the stride: U |o|.  dd_k = 0 without DFL.
                  |d cx| <= (stride / 2) (dd0 + dd2 + U (|x1| + |x2| + |x1 + x2|)) + U |cx|
                  |d w|  <=  stride      (dd0 + dd2 + U (|x1| + |x2| + |x2 - x1|)) + U |w|             (cy, h likewise)
  DFL         m = max of the side's 17 logits (exact), e_i = expf(fl(z_i - m)), S = sum e_i (sequential), dist = sum fl(fl(e_i / S) i)
              (sequential).  As in detect_ref a relative error eps_i of e_i acts like a logit error log(1 + eps_i) and m cancels:
                  |dist' - dist| <= e^(2 D) sum_i s_i |i - dist| eta_i,   D = max eta_i <= detect_ref.DZ_MAX (asserted),
                  eta_i = U |z_i - m| (the argument's rounding) + 2 U (expf within 1 ulp)                      -- 17 exponentials
              Errors common to every term or proportional to it, relative on dist (all terms are positive):
                  the 17-term float32 sum S: 16 adds, 16 U;   17 divisions: U each;   the products with i: U each;   the 17-term
                  accumulation: 16 adds, 16 U (every partial sum is at most dist)   -- 34 U, taken as DFL_SUMS = 36 U dist with the second
                  order of 1 / (1 - 16 U).
              Flushed values: an e_i below 2^-126 may come back zero or with fewer bits, at most 2^-126 absolute against S >= 1, 17 bins,
              |i - dist| <= 16; a quotient below 2^-126 likewise, times i, sum of i = 136:  DFL_FLUSH = 2^-116 grid units, absolute.
                  dd = e^(2 D) sum_i s_i |i - dist| eta_i + DFL_SUMS U dist + DFL_FLUSH

Every constant above is derived from the code; the one measured constant is conv_ref.K_CONV inside dz.  "expf / v_exp_f32 / v_rcp_f32
within 1 ulp" are the stated accuracies conv_ref.py and detect_ref.py already rest on.

The yardsticks.  v5_f32, v6_f32 restate the decodes in NumPy float32: every exp / exp2 and fast reciprocal result moved to one of the
two float32 neighbours of the exact value at random (detect_ref.within_one_ulp, _exp_f32), sums strictly sequential, products and adds
rounded separately.  *_yardstick divide their error by the bound (at dz = |float32(z) - z| for logits that are no float32).  Worst
ratios over tests/test_detect56_ref_cpu.py's synthetic operands (G1, G2, G3, every width, the stress logits) -- YARD56 below, which that
test reproduces and holds to within 15 % below; every GPU case re-measures the ratio on its own fetched operands and asserts <= 1.

The old criterion.  old_criterion is what tests/test_gpu_v6.py (and the v5 / v7 network tests alike) assert of a whole network's head:
boxes within atol + rtol |want| and probabilities within a flat tolerance, per precision."""
import numpy as np

import detect_ref as D
from ops_ref import EPS32

U = EPS32
F32 = np.float32
MARGIN = D.MARGIN
SIG_FLUSH = 2.0 ** -126
SIG56_Z_MAX = 1000.0
DFL_BINS = 17
DFL_SUMS = 36.0
DFL_FLUSH = 2.0 ** -116
FORMS = D.FORMS
# recorded worst ratios of the restatements (box columns, probability columns); tests/test_detect56_ref_cpu.py reproduces them
YARD56 = {"v5-exact": (0.762, 0.829), "v5-fast": (0.683, 0.910), "v6": (0.877, 0.817), "v6-dfl": (0.132, 0.800)}
OLD_TOL = {"fp32": (1e-3, 1e-5, 1e-3), "fp16": (0.1, 1e-2, 2e-2), "bf16": (1.0, 8e-2, 1.5e-1), "fp16x3": (1e-3, 1e-5, 1e-4)}     # atol, rtol (boxes), probabilities


def _flat(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], a.shape[1], -1)


def cells(sizes):
    return [h * w for h, w in sizes]


def v5_row_off(sizes):
    hw = cells(sizes)
    return [0, 3 * hw[0], 3 * (hw[0] + hw[1])]


def v6_row_off(sizes):
    hw = cells(sizes)
    return [0, hw[0], hw[0] + hw[1]]


def sigmoid_ref(z, dz, form):
    """(p, its absolute bound ds) of a float64 logit array with slack dz (module docstring: sigmoid)."""
    z = np.asarray(z, np.float64)
    assert np.abs(z).max() + np.max(dz) <= SIG56_Z_MAX, "the sigmoid bound is stated for |z| <= %g, this case has %g" % (SIG56_Z_MAX, np.abs(z).max())
    with np.errstate(over="ignore", under="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
        q = 1.0 / (1.0 + np.exp(z))                                          # 1 - p without cancellation
    rel = 2 * U * q + 2 * U if form == "exact" else 2 * U * (np.abs(z) + 1) * q + 3 * U
    return p, p * q * dz * np.exp(2 * dz) + rel * p + SIG_FLUSH


# ------------------------------------------------------------------------------------------------------------------------- v5 layout
def v5_rows(z, no):
    """Per-level (B, 3 no, hw) -> (B, A, no) in the head's row order, by reshapes alone: level, anchor, cell."""
    out = []
    for zl in z:
        B, c, hw = zl.shape
        assert c == 3 * no
        out.append(zl.reshape(B, 3, no, hw).transpose(0, 1, 3, 2).reshape(B, 3 * hw, no))
    return np.concatenate(out, 1)


def _v5_geometry(sizes, strides, anchors):
    """Per row of the head: (x, y, stride, anchor w, anchor h), float64, from integers."""
    anchors = np.asarray(anchors, np.float64).reshape(3, 3, 2)
    cols = []
    for l, (h, w) in enumerate(sizes):
        p = np.tile(np.arange(h * w), 3)
        a = np.repeat(np.arange(3), h * w)
        cols.append(np.stack([p % w, p // w, np.full(p.shape, float(strides[l])), anchors[l, a, 0], anchors[l, a, 1]], 0))
    return np.concatenate(cols, 1)


def v5_ref(z, dz, sizes, strides, anchors, form):
    """(want, bound), each (B, A, no): z[l] (B, 3 no, hw_l) float64 logits, dz[l] their slack (None: the logits ARE the operands)."""
    assert form in FORMS, form
    no = z[0].shape[1] // 3
    zr = v5_rows([np.asarray(a, np.float64) for a in z], no)
    dzr = np.zeros_like(zr) if dz is None else v5_rows([np.asarray(a, np.float64) for a in dz], no)
    s, ds = sigmoid_ref(zr, dzr, form)
    gx, gy, st, aw, ah = _v5_geometry(sizes, strides, anchors)
    want, bound = s.copy(), ds.copy()
    for c, g in ((0, gx), (1, gy)):
        t1 = 2 * s[..., c] - 0.5
        want[..., c] = (t1 + g) * st
        bound[..., c] = st * (2 * ds[..., c] + U * np.abs(t1) + U * np.abs(t1 + g)) + U * np.abs(want[..., c])
    for c, an in ((2, aw), (3, ah)):
        t, dt = 2 * s[..., c], 2 * ds[..., c]
        want[..., c] = t * t * an
        bound[..., c] = an * (2 * t * dt + dt * dt + SIG_FLUSH) + 2 * U * np.abs(want[..., c]) + SIG_FLUSH
    return want, MARGIN * bound


def v5_head_ref(feats, w, b, sizes, strides, anchors, prec, info=None):
    """The fused kernel's head from the fetched 16-bit feature maps (B, cin, h, w), the weights as stored (3 no, cin, 1, 1) and the
    float32 biases; info receives the float64 logits and their slack."""
    z, dz = [], []
    for l in range(3):
        zl, dl = D.logits_ref(feats[l], w[l], b[l], prec)
        z.append(zl)
        dz.append(dl)
    if info is not None:
        info.update(z=z, dz=dz, form="fast", max_logit=max(float(np.abs(a).max()) for a in z), min_z=min(float(a.min()) for a in z),
                    max_z=max(float(a.max()) for a in z), max_dz=max(float(a.max()) for a in dz))
    return v5_ref(z, dz, sizes, strides, anchors, "fast")


def v5_logits_ref(logits, sizes, strides, anchors, info=None):
    """The entry for detect_v5_kernel: fetched float32 logits, NCHW per level -- no slack, exact form."""
    z = [_flat(a).astype(np.float64) for a in logits]
    if info is not None:
        info.update(z=z, dz=None, form="exact", max_logit=max(float(np.abs(a).max()) for a in z), min_z=min(float(a.min()) for a in z),
                    max_z=max(float(a.max()) for a in z), max_dz=0.0)
    return v5_ref(z, None, sizes, strides, anchors, "exact")


def _sigmoid_f32(z, form, rng):
    one = F32(1)
    d = (one + D._exp_f32((-z).astype(F32), form, rng)).astype(F32)
    if form == "exact":
        return (one / d).astype(F32)
    r = D.within_one_ulp(1.0 / d.astype(np.float64), rng)
    return np.where(r < F32(2.0 ** -126), F32(0), r).astype(F32)              # v_rcp_f32 returns no subnormal


def v5_f32(z, sizes, strides, anchors, form, seed=0, half=0.5, swap_xy=False):
    """The v5 decode in NumPy float32 on float32 logits z[l] (B, 3 no, hw) (module docstring: the yardsticks).  half / swap_xy are the
    knobs two of tests/test_detect56_ref_cpu.py's wrong kernels need; a kernel has neither."""
    rng = np.random.default_rng(seed)
    no = z[0].shape[1] // 3
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        s = _sigmoid_f32(v5_rows([np.asarray(a, F32) for a in z], no), form, rng)
        gx, gy, st, aw, ah = [a.astype(F32) for a in _v5_geometry(sizes, strides, anchors)]
        if swap_xy:
            gx, gy = gy, gx
        out = s.copy()
        two = F32(2)
        for c, g in ((0, gx), (1, gy)):
            out[..., c] = ((((s[..., c] * two).astype(F32) - F32(half)).astype(F32) + g).astype(F32) * st).astype(F32)
        for c, an in ((2, aw), (3, ah)):
            t = (s[..., c] * two).astype(F32)
            out[..., c] = ((t * t).astype(F32) * an).astype(F32)
    assert out.dtype == F32
    return out


def v5_yardstick(z, sizes, strides, anchors, form, seed=0):
    """(worst |f32 - f64| / bound over the box columns, over the probability columns) of v5_f32 on float32(z), the bound taken at the
    rounding's own dz = |float32(z) - z| (zero for logits that are float32 already)."""
    z64 = [np.asarray(a, np.float64) for a in z]
    z32 = [a.astype(F32) for a in z64]
    want, bound = v5_ref(z64, [np.abs(a - b) for a, b in zip(z32, z64)], sizes, strides, anchors, form)
    _, rb, rp = check(v5_f32(z32, sizes, strides, anchors, form, seed), want, bound)
    return rb, rp


# ------------------------------------------------------------------------------------------------------------------------- v6
def _dfl_ref(zr):
    """(dist, its bound dd) of (B, 68, hw) float64 logits: (B, 4, hw) each."""
    B, c, hw = zr.shape
    assert c == 4 * DFL_BINS
    z = zr.reshape(B, 4, DFL_BINS, hw)
    x = z - z.max(2, keepdims=True)
    e = np.exp(x)
    s = e / e.sum(2, keepdims=True)
    k = np.arange(float(DFL_BINS)).reshape(1, 1, DFL_BINS, 1)
    dist = (s * k).sum(2)
    eta = U * np.abs(x) + 2 * U
    Dm = eta.max(2)
    assert Dm.max() <= D.DZ_MAX, "the DFL bound is stated for exponent errors up to %g, this case has %g" % (D.DZ_MAX, Dm.max())
    return dist, np.exp(2 * Dm) * (s * np.abs(k - dist[:, :, None]) * eta).sum(2) + DFL_SUMS * U * dist + DFL_FLUSH


def v6_ref(reg, cls, sizes, strides, dfl):
    """(want, bound), each (B, A, 5 + nc), from the fetched float32 reg (B, 4 | 68, h, w) and class logits (B, nc, h, w) per level."""
    wants, bounds = [], []
    for l, (h, w) in enumerate(sizes):
        r64, c64 = _flat(reg[l]).astype(np.float64), _flat(cls[l]).astype(np.float64)
        B = r64.shape[0]
        if dfl:
            d, dd = _dfl_ref(r64)
        else:
            assert r64.shape[1] == 4
            d, dd = r64, np.zeros_like(r64)
        ax, ay = (np.arange(h * w) % w) + 0.5, (np.arange(h * w) // w) + 0.5
        x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
        st = float(strides[l])
        box = np.stack([(x1 + x2) / 2 * st, (y1 + y2) / 2 * st, (x2 - x1) * st, (y2 - y1) * st], 2)          # (B, hw, 4)
        rx, ry = U * (np.abs(x1) + np.abs(x2)), U * (np.abs(y1) + np.abs(y2))
        bbox = np.stack([st / 2 * (dd[:, 0] + dd[:, 2] + rx + U * np.abs(x1 + x2)), st / 2 * (dd[:, 1] + dd[:, 3] + ry + U * np.abs(y1 + y2)),
                         st * (dd[:, 0] + dd[:, 2] + rx + U * np.abs(x2 - x1)), st * (dd[:, 1] + dd[:, 3] + ry + U * np.abs(y2 - y1))], 2) + U * np.abs(box)
        p, dp = sigmoid_ref(c64, 0.0, "exact")
        one = np.ones((B, h * w, 1))
        wants.append(np.concatenate([box, one, p.transpose(0, 2, 1)], 2))
        bounds.append(np.concatenate([MARGIN * bbox, 0 * one, MARGIN * dp.transpose(0, 2, 1)], 2))
    return np.concatenate(wants, 1), np.concatenate(bounds, 1)


def v6_f32(reg, cls, sizes, strides, dfl, seed=0, half=0.5, order=(0, 1, 2, 3), xyxy=False, obj=1.0, first_row_level=False,
           bins=None, nbins=DFL_BINS, side_stride=DFL_BINS, use_max=True):
    """The v6 decodes in NumPy float32 on the float32 operands (module docstring: the yardsticks).  Everything behind `seed` is a knob one
    of tests/test_detect56_ref_cpu.py's wrong kernels needs; a kernel has none.  first_row_level: the rows of a 32-row block take the
    grid width and stride of the block's first row's level."""
    rng = np.random.default_rng(seed)
    hw, off = cells(sizes), v6_row_off(sizes)
    kk = np.arange(DFL_BINS, dtype=F32) if bins is None else np.asarray(bins, F32)
    rows = []
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for l, (h, w) in enumerate(sizes):
            r, c = _flat(reg[l]).astype(F32), _flat(cls[l]).astype(F32)
            B = r.shape[0]
            if dfl:
                z = np.stack([r[:, k * side_stride:k * side_stride + nbins] for k in range(4)], 1)          # (B, 4, nbins, hw)
                x = (z - z.max(2, keepdims=True)).astype(F32) if use_max else z
                e = D._exp_f32(x, "exact", rng)
                se = np.zeros((B, 4, h * w), F32)
                for i in range(nbins):
                    se = (se + e[:, :, i]).astype(F32)
                d = np.zeros((B, 4, h * w), F32)
                for i in range(nbins):
                    d = (d + ((e[:, :, i] / se).astype(F32) * kk[i]).astype(F32)).astype(F32)
            else:
                d = r
            d = d[:, list(order)]
            row = off[l] + np.arange(h * w)
            nx, st = np.full(h * w, w), np.full(h * w, strides[l])
            if first_row_level:
                l0 = np.searchsorted(np.asarray(off), row // 32 * 32, "right") - 1
                nx, st = np.asarray([s_[1] for s_ in sizes])[l0], np.asarray(strides)[l0]
            p = np.arange(h * w)
            ax, ay = ((p % nx).astype(F32) + F32(half)).astype(F32), ((p // nx).astype(F32) + F32(half)).astype(F32)
            st = st.astype(F32)
            x1, y1, x2, y2 = (ax - d[:, 0]).astype(F32), (ay - d[:, 1]).astype(F32), (ax + d[:, 2]).astype(F32), (ay + d[:, 3]).astype(F32)
            two = F32(2)
            if xyxy:
                box = np.stack([x1 * st, y1 * st, x2 * st, y2 * st], 2).astype(F32)
            else:
                box = np.stack([(x1 + x2).astype(F32) / two * st, (y1 + y2).astype(F32) / two * st, (x2 - x1).astype(F32) * st, (y2 - y1).astype(F32) * st], 2).astype(F32)
            pr = _sigmoid_f32(c, "exact", rng).transpose(0, 2, 1)
            rows.append(np.concatenate([box, np.full((B, h * w, 1), obj, F32), pr], 2))
    out = np.concatenate(rows, 1)
    assert out.dtype == F32
    return out


def v6_yardstick(reg, cls, sizes, strides, dfl, seed=0):
    """(worst |f32 - f64| / bound over the box columns, over the class columns) of v6_f32 on the float32 operands themselves."""
    want, bound = v6_ref(reg, cls, sizes, strides, dfl)
    _, rb, rp = check(v6_f32(reg, cls, sizes, strides, dfl, seed), want, bound)
    return rb, rp


# ------------------------------------------------------------------------------------------------------------------------- the checks
def ratios(got, want, bound):
    """|got - want| / bound per element: 0 where they agree exactly, inf where the bound is 0 and they do not, or got is no number."""
    g = np.asarray(got, np.float64)
    err = np.abs(g - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return np.where(np.isfinite(g), r, np.inf)


def check(got, want, bound):
    """(ok per element, worst |err| / bound over the box columns 0..3, over the columns 4..).  NaN / inf are never ok; a column whose
    bound is zero (v6's objectness) is compared for equality."""
    assert np.shape(got) == want.shape, (np.shape(got), want.shape)
    r = ratios(got, want, bound)
    return r <= 1.0, float(r[..., :4].max()), float(r[..., 4:].max())


def old_criterion(got, want, prec, obj_one=False):
    """What the whole-network tests assert of a head (tests/test_gpu_v6.py): every box column within atol + rtol |want|, every other
    column within a flat tolerance, per precision; obj_one: column 4 equal to 1.0 as well (the v6 tests)."""
    atol, rtol, ptol = OLD_TOL[prec]
    g = np.asarray(got, np.float64)
    if not np.isfinite(g).all() or (obj_one and not (g[..., 4] == 1.0).all()):
        return False
    return bool((np.abs(g[..., :4] - want[..., :4]) <= atol + rtol * np.abs(want[..., :4])).all() and np.abs(g[..., 4:] - want[..., 4:]).max() <= ptol)
