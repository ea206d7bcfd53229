"""Per-element checker and float64 references for the operators between the convolutions (csrc/aux_kernels.hip, csrc/fuse_ops.hip):
max-pool / upsample / depth-to-space / shuffle / input (exact), avg-pool / weighted sum / scale (fp32 arithmetic, one store rounding),
the squeeze-and-excitation gate (fp32 throughout).  No GPU and no project code in here: torch / NumPy only, tested by
tests/test_ops_ref_cpu.py, used by tests/test_gpu_ops_exact.py.

The bound of an element is  |got - want64| <= R_prec(want64) + slack:
  R      the store rounding of the engine precision (half an ulp of the storage type at the reference value; zero in fp32 mode),
  slack  k * 2^-24 * S for the fp32 arithmetic in front of the store, S = the sum of the magnitudes that enter the element.
k is not tuned on a device: it is four times the worst |f32 - f64| / (2^-24 S) of a NumPy float32 restatement of the kernel's
expression, in the kernel's order, against float64 (the "yardstick"), at least 4.  The measured yardstick ratios stand next to the
constants below; the GPU tests re-measure them on their own fetched inputs and assert that the constants still cover them."""
import numpy as np
import torch
import torch.nn.functional as F

PRECISIONS = ("fp32", "fp16", "bf16", "fp16x3")
EPS32 = 2.0 ** -24      # half an ulp of fp32 relative to the binade: one fp32 rounding is at most EPS32 * |value|

# activation ids of models.py (ACT_*); the GPU test asserts that they agree
ACT_NONE, ACT_SILU, ACT_RELU, ACT_LEAKY, ACT_HSWISH, ACT_HSIGMOID, ACT_RELU6 = range(7)
ACT_NAMES = {ACT_NONE: "none", ACT_SILU: "silu", ACT_RELU: "relu", ACT_LEAKY: "leaky", ACT_HSWISH: "hswish", ACT_HSIGMOID: "hsigmoid", ACT_RELU6: "relu6"}

# ---- yardstick constants: k = max(4, 4 * worst ratio), ratio = |numpy f32 restatement - f64| / (2^-24 S).
# YARD_*: the worst ratio over all cases -- every GPU case re-measures it on its own fetched inputs (a CPU computation: NumPy float32
# against float64; printed per case) and asserts that it stays inside, and test_ops_ref_cpu.py measures it on synthetic inputs of the
# same distributions in all four storage roundings (avg-pool 3.18, wsum 3.31, scale 0.99) and holds it to within 15 % below:
#   avg-pool  (k*k sequential adds, one multiply by fl(1 / k^2))
#   wsum      (<= 3 products, <= 2 adds, the activation; SiLU = v / (1 + exp(-v)) in float32)
#   scale     (one multiply: at most one rounding)
YARD_AVG = 3.5670
YARD_WSUM = 3.8684
YARD_SCALE = 1.0
K_AVG = max(4.0, 4 * YARD_AVG)
K_WSUM = max(4.0, 4 * YARD_WSUM)
K_SCALE = max(4.0, 4 * YARD_SCALE)
GATE_FLOOR = 2.0 ** -22   # a gate lies in (0, 1): four fp32 half-ulps at 1


# ------------------------------------------------------------------------------------------------------------------ the checker
def _floor_log2(a):
    """floor(log2 |a|) exactly (frexp, no rounding of a logarithm); -inf-free: zeros map to a very small exponent."""
    a = np.abs(np.asarray(a, np.float64))
    m, e = np.frexp(a)            # a = m 2^e, 0.5 <= m < 1
    return np.where(a > 0, e - 1, -2000)


def ulp16(v):
    """Spacing of IEEE half at |v|: 2^(max(floor(log2 |v|), -14) - 10)."""
    return np.ldexp(1.0, np.maximum(_floor_log2(v), -14) - 10)


def ulpbf(v):
    """Spacing of bfloat16 at |v|: 2^(max(floor(log2 |v|), -126) - 7)."""
    return np.ldexp(1.0, np.maximum(_floor_log2(v), -126) - 7)


def store_bound(want64, prec):
    """R_prec(want): the largest error a correctly rounded store of `want` into the engine precision's storage type can leave."""
    w = np.asarray(want64, np.float64)
    if prec == "fp32":
        return np.zeros_like(w)
    if prec == "fp16":
        return ulp16(w) / 2
    if prec == "bf16":
        return ulpbf(w) / 2
    if prec == "fp16x3":
        # hi = half(x), lo = half((x - hi) 2^11): 2^-11 relative on a residual of at most 2^-11 |x|; below 2^-14 the whole value sits
        # in lo, whose half-ulp is at most 2^-26 after the 2^-11 scale
        return 2.0 ** -22 * np.abs(w) + 2.0 ** -26
    raise ValueError(prec)


def round_ok(got, want64, prec, slack):
    """Boolean array: |got - want64| <= R_prec(want64) + slack, element by element (NaN / inf in got are never ok)."""
    g = np.asarray(got, np.float64)
    w = np.asarray(want64, np.float64)
    return np.isfinite(g) & (np.abs(g - w) <= store_bound(w, prec) + slack)


def worst(got, want64, prec, slack):
    """(worst |err| / bound over the elements, worst |err|): the figure the GPU tests print.  A zero bound with zero error counts 0."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want64, np.float64))
    bound = store_bound(want64, prec) + slack
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0, float(err.max()) if err.size else 0.0


def yardstick_ratio(f32, f64, S):
    """worst |f32 - f64| / (2^-24 S) of a float32 restatement against float64 (elements with S = 0 must be exact)."""
    err = np.abs(np.asarray(f32, np.float64) - np.asarray(f64, np.float64))
    S = np.asarray(S, np.float64)
    assert (err[S == 0] == 0).all()
    return float((err[S > 0] / (EPS32 * S[S > 0])).max()) if (S > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------------------- storage roundings
def x3_split(v):
    """NumPy restatement of x3_split (csrc/elem16.h): hi = half(x), no subnormal hi; lo = half((x - hi) * 2048).  v: float32."""
    v = np.asarray(v, np.float32)
    h = v.astype(np.float16)
    h = np.where(np.abs(v) >= np.float32(6.103515625e-05), h, np.float16(0))
    l = ((v - h.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return h, l


def x3_join(h, l):
    """x3_join (csrc/elem16.h): float(hi) + float(lo) * 2^-11, in float32."""
    return h.astype(np.float32) + l.astype(np.float32) * np.float32(1.0 / 2048.0)


def storage_round(v, prec):
    """A float32 array as the engine precision stores it (round to nearest even), returned as float32."""
    v = np.ascontiguousarray(v, np.float32)
    if prec == "fp32":
        return v.copy()
    if prec == "fp16":
        with np.errstate(over="ignore"):
            return v.astype(np.float16).astype(np.float32)
    if prec == "bf16":
        return torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    if prec == "fp16x3":
        return x3_join(*x3_split(v))
    raise ValueError(prec)


def bf16_truncate(v):
    """bfloat16 by dropping the low 16 bits (what a store WITHOUT rounding does): the mistake the checker has to see."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return u.view(np.float32)


# ------------------------------------------------------------------------------------------------------------- float64 references
def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def maxpool_ref(x, k, s, p):
    """torch.nn.MaxPool2d(k, s, p) (-inf padding) of an NCHW array, in float64."""
    return F.max_pool2d(_t64(x), k, s, p).numpy()


def avgpool_ref(x, k, s, p):
    """F.avg_pool2d(x, k, s, p, ceil_mode=False, count_include_pad=True) in float64, and S = avg-pool of |x| (sum |x| / k^2)."""
    return F.avg_pool2d(_t64(x), k, s, p, False, True).numpy(), F.avg_pool2d(_t64(np.abs(x)), k, s, p, False, True).numpy()


def avgpool_f32(x, k, s, p):
    """The kernel's order in NumPy float32: the window's taps in row-major order added into a float32 sum (padding taps add nothing),
    then one multiply by fl(1 / (k * k))."""
    x = np.asarray(x, np.float32)
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = np.zeros((B, C, H + 2 * p + s, W + 2 * p + s), np.float32)
    xp[:, :, p:p + H, p:p + W] = x
    acc = np.zeros((B, C, Ho, Wo), np.float32)
    for r in range(k):
        for q in range(k):
            acc = acc + xp[:, :, r:r + (Ho - 1) * s + 1:s, q:q + (Wo - 1) * s + 1:s]
    return acc * (np.float32(1.0) / np.float32(k * k))


def upsample2_ref(x):
    """Nearest 2x: out[2y + dy][2x + dx] = in[y][x]."""
    return np.repeat(np.repeat(np.asarray(x), 2, 2), 2, 3)


def depth2space_ref(x):
    """aux_kernels.hip: out[2y + dy][2x + dx][c] = in[y][x][(2 dy + dx) C + c], on NCHW arrays (4C -> C channels)."""
    x = np.asarray(x)
    B, C4, H, W = x.shape
    assert C4 % 4 == 0
    C = C4 // 4
    out = np.empty((B, C, 2 * H, 2 * W), x.dtype)
    for dy in range(2):
        for dx in range(2):
            out[:, :, dy::2, dx::2] = x[:, (2 * dy + dx) * C:(2 * dy + dx + 1) * C]
    return out


def shuffle_ref(x, groups):
    """torch channel_shuffle(x, groups) by its definition: view(B, g, C / g, H, W).transpose(1, 2).reshape(B, C, H, W)."""
    x = np.asarray(x)
    B, C, H, W = x.shape
    assert C % groups == 0
    return np.ascontiguousarray(x.reshape(B, groups, C // groups, H, W).transpose(0, 2, 1, 3, 4)).reshape(B, C, H, W)


_ACT_MODULES = {ACT_SILU: torch.nn.SiLU(), ACT_RELU: torch.nn.ReLU(), ACT_LEAKY: torch.nn.LeakyReLU(0.1), ACT_HSWISH: torch.nn.Hardswish(),
                ACT_HSIGMOID: torch.nn.Hardsigmoid(), ACT_RELU6: torch.nn.ReLU6()}


def act_ref(v, act):
    """The activation's torch module on float64."""
    return np.asarray(v, np.float64) if act == ACT_NONE else _ACT_MODULES[act](_t64(v)).numpy()


def act_f32(v, act):
    """The kernel's expression (fuse_ops.hip wsum_kernel) in NumPy float32."""
    v = np.asarray(v, np.float32)
    one, three, six, zero = np.float32(1), np.float32(3), np.float32(6), np.float32(0)
    if act == ACT_NONE:
        return v
    if act == ACT_SILU:
        with np.errstate(over="ignore"):
            return v / (one + np.exp(-v))
    if act == ACT_RELU:
        return np.maximum(v, zero)
    if act == ACT_LEAKY:
        return np.maximum(v, np.float32(0.1) * v)
    if act == ACT_HSWISH:
        return v * np.minimum(np.maximum(v + three, zero), six) / six
    if act == ACT_HSIGMOID:
        return np.minimum(np.maximum(v + three, zero), six) / six
    if act == ACT_RELU6:
        return np.minimum(np.maximum(v, zero), six)
    raise ValueError(act)


def _full(v, hw):
    """An input of half the output's resolution is read at (y >> 1, x >> 1)."""
    return v if tuple(v.shape[2:]) == tuple(hw) else upsample2_ref(v)


def wsum_ref(ins, weights, act):
    """act(sum_i w_i x_i) in float64 (weights as the float32 values the graph stores).  Returns (want, S, pre-activation sum).
    S = sum_i |w_i x_i|, plus 3 for the hard-sigmoid (the constant of relu6(v + 3) / 6 enters that element: at v = 0 the result is 0.5
    with nothing else to scale its fp32 roundings by; hard-swish multiplies by v, so every error term scales with |v| <= S)."""
    hw = max(tuple(v.shape[2:]) for v in ins)
    w = [float(np.float32(x)) for x in weights]
    pre = sum(wi * _full(np.asarray(v, np.float64), hw) for wi, v in zip(w, ins))
    S = sum(abs(wi) * np.abs(_full(np.asarray(v, np.float64), hw)) for wi, v in zip(w, ins))
    if act == ACT_HSIGMOID:
        S = S + 3.0
    return act_ref(pre, act), S, pre


def wsum_f32(ins, weights, act):
    """The kernel's order in NumPy float32: acc = 0; acc = w_k * x_k + acc for k = 0, 1, 2 (two roundings where the kernel's fma has
    one: the restatement is never more accurate than the kernel's form); then the activation."""
    hw = max(tuple(v.shape[2:]) for v in ins)
    acc = np.zeros(_full(np.asarray(ins[0]), hw).shape, np.float32)
    for wi, v in zip(weights, ins):
        acc = np.float32(wi) * _full(np.asarray(v, np.float32), hw) + acc
    return act_f32(acc, act)


def _hidden_ref(v, hidden_act):
    return np.maximum(v, 0.0) if hidden_act == ACT_RELU else v / (1.0 + np.exp(-v))


def se_gate_ref(x, W1, b1, W2, b2, hidden_act=ACT_SILU, gate_act=ACT_NONE):
    """gate[n][c] = sigmoid | hardsigmoid (W2 silu | relu (W1 mean_hw(x[n]) + b1) + b2) in float64: F.adaptive_avg_pool2d + two matmuls."""
    m = F.adaptive_avg_pool2d(_t64(x), 1).numpy()[:, :, 0, 0]                       # (B, C)
    W1, W2 = np.asarray(W1, np.float64).reshape(len(b1), -1), np.asarray(W2, np.float64).reshape(len(b2), -1)
    h = _hidden_ref(m @ W1.T + np.asarray(b1, np.float64), hidden_act)
    v = h @ W2.T + np.asarray(b2, np.float64)
    return act_ref(v, ACT_HSIGMOID) if gate_act == ACT_HSIGMOID else torch.sigmoid(_t64(v)).numpy()


def se_gate_f32(x, W1, b1, W2, b2, hidden_act=ACT_SILU, gate_act=ACT_NONE):
    """The gate in NumPy float32: the channel mean as a sum over the pixels in index order divided by H * W, the two products, exp."""
    x = np.asarray(x, np.float32)
    B, C, H, W = x.shape
    flat = x.reshape(B, C, H * W)
    acc = np.zeros((B, C), np.float32)
    for p in range(H * W):
        acc = acc + flat[:, :, p]
    m = acc / np.float32(H * W)
    W1, W2 = np.asarray(W1, np.float32).reshape(len(b1), -1), np.asarray(W2, np.float32).reshape(len(b2), -1)
    v = (m @ W1.T + np.asarray(b1, np.float32)).astype(np.float32)
    h = np.maximum(v, np.float32(0)) if hidden_act == ACT_RELU else v / (np.float32(1) + np.exp(-v))
    v = (h @ W2.T + np.asarray(b2, np.float32)).astype(np.float32)
    if gate_act == ACT_HSIGMOID:
        return act_f32(v, ACT_HSIGMOID)
    return np.float32(1) / (np.float32(1) + np.exp(-v))
