"""Float64 reference and per-element bound of ONE conv layer  y = act(conv(x, w) + b [+ r])  |  act(conv(x, w) + b) + r  (csrc/conv_*.hip,
conv_fc.hip, conv_stem*.hip), built on tests/ops_ref.py.  No GPU and no project code in here: torch / NumPy only, tested by
tests/test_conv_ref_cpu.py, used by tests/test_gpu_conv_exact.py.

Operands.  x (and the residual r) are the values the layer reads, exact values of the storage type (a joined fp16x3 pair fits float32);
w is the float32 weight rounded the way the engine stores it -- `ops_ref.storage_round`: every packing kernel of the 16-bit modes converts
with round to nearest even (pack_weights_*_kernel through stf, Bf16 / Fp16::host_from_f32 on the host side), the split precision packs
x3_split(w) (pack_weights_x3_kernel, pack_weights_h8x3_kernel), fp32 mode keeps the float32; b stays float32 in every mode.

The bound of an element is  |got - want| <= R_prec(want) + slack,  slack = K_CONV 2^-24 S + X3(prec) + A(prec, act):
  want    the expression in float64 on those operands (torch conv2d in float64, the activation in float64),
  R       ops_ref.store_bound: half an ulp of the storage type; zero in fp32 mode and for a layer with a float32 output in any mode,
  S       conv(|x|, |w|) + |b| + |r|: the sum of the magnitudes that enter the element,
  K_CONV  four times the worst |f32 - f64| / (2^-24 S) of a float32 restatement of the whole expression on the same operands (the
          yardstick; at least 4): the worse of torch's float32 conv2d and a strictly sequential float32 accumulation in tap-major,
          channel-minor order (one rounding per product, one per add: never more accurate than an fma chain), bias, residual and
          activation in float32 behind it.  A CPU figure; no device value enters it,
  X3      the product term the split precision drops (below),
  A       the activation's own error in front of the store (below)."""
import numpy as np
import torch
import torch.nn.functional as F

import ops_ref as R
from ops_ref import ACT_NONE, ACT_SILU, ACT_RELU, ACT_LEAKY, EPS32

RES_NONE, RES_AFTER_ACT, RES_BEFORE_ACT = 0, 1, 2     # models.py (the GPU test asserts that they agree)

# ---- the yardstick.  YARD_CONV: the worst ratio over tests/test_conv_ref_cpu.py's synthetic layers (K = 16 ... 4608: 9 * 16 ... 9 * 512, 1 * 2048
# and the short sums of the pointwise, stem and generic cases on large maps; all four storage roundings, every activation and residual
# mode): torch's float32 conv2d 6.082 (K = 147 behind SiLU), the sequential accumulation 4.819.  That test reproduces the figure and holds
# it to within 15 % below the constant.  Every GPU case re-measures the ratio on its own fetched inputs (a CPU computation), prints it
# and asserts that it stays inside: the worst of the single-layer cases is 6.969 (ig128x64-m in fp32 mode: K = 72 behind leaky ReLU, a million
# elements); the stages of the fused launches (tests/fused_ref.py) are measured by the same rule, and cv1 of the C2f chain of
# tests/test_fused_ref_cpu.py (1x1, K = 32 behind SiLU, fp16 operands +-2) reaches 6.983, which is the recorded figure.
YARD_CONV = 6.99
K_CONV = max(4.0, 4 * YARD_CONV)
YARD_SAMPLE = 4096      # output elements of the sequential restatement per case (fixed seed); the torch one covers all of them

# ---- the split precision's dropped term.  A stored pair is the value a = a_hi + 2^-11 a_lo exactly; the kernels compute
#     a w = a_hi w_hi + 2^-11 (a_hi w_lo + a_lo w_hi)                                                            (elem16.h)
# and drop 2^-22 a_lo w_lo.  For a normal hi half (|a| >= 2^-14): |a - a_hi| <= 2^-11 |a| (round to nearest, 11 significant bits) and
# the lo half's own rounding moves it by at most 2^-11 of that, so t(a) := |2^-11 a_lo| <= 2^-11 (1 + 2^-11) |a_hi| and, with
# |a_hi| <= |a| + t(a):  t(a) <= 2^-11 (1 + 2^-10) |a|.  Below 2^-14 hi is zero and the whole value sits in lo: t(a) = |a|.  The dropped
# term of an element is at most  sum t(x) t(w)  = conv(t(x), t(w)) -- for normal operands (1 + 2^-10)^2 2^-22 conv(|x|, |w|) < 1.002 * 2^-22 S;
# it is evaluated as that convolution so that half-subnormal operands (which lose up to 2^-11 of their product) are covered without a floor.
X3_T = 2.0 ** -11 * (1 + 2.0 ** -10)

# ---- A(prec, act): the activation's own error, as a relative error on |act(v)| (v: the activation's argument).  Zero for none, ReLU
# and leaky ReLU (a selection, or one multiply whose rounding the yardstick's restatement has too).  SiLU, first order in 2^-24:
#   16-bit modes (elem16.h silu_for<16-bit>: v * v_rcp_f32(1 + __expf(-v)), __expf(x) = v_exp_f32(x * log2 e)):
#       t = fl(-v * fl(log2 e)): the constant's and the product's rounding, 2 * 2^-24 |t| absolute, which exp2 turns into a RELATIVE error
#         of 2 * 2^-24 |t| ln 2 = 2^-23 |v| on e = exp(-v);  v_exp_f32: 1 ulp <= 2^-23 relative on e
#       d = fl(1 + e): 2^-24;  the error of e enters d scaled by e / (1 + e) <= 1
#       v_rcp_f32: 1 ulp <= 2^-23;  the product v * q: 2^-24
#     sum: 2^-23 (|v| + 1) + 2^-24 + 2^-23 + 2^-24 = 2^-23 (|v| + 3).  At |v| = 20 that is 2.7e-6 relative, 90 times below half an ulp of
#     IEEE half (2^-12) and 700 times below bfloat16's (2^-9).  Valid while exp(-v) is a normal float: |v| <= 80 (asserted by the caller).
#   fp16x3 (elem16.h x3_silu: compensated product, exp2, one Newton step on the reciprocal; no growth with |v|: the product's rounding
#     error is carried in r):  v_exp_f32 2^-23;  e * r and the fma that applies it: 2 * 2^-24;  d: 2^-24;  the refined reciprocal: 2^-24;
#     v * q: 2^-24.  Sum 3 * 2^-23 = 3.58e-7.  elem16.h states 3.2e-7 as the maximum it measured on its NumPy model
#     (tests/test_x3_silu_model.py); the same model reaches 3.4e-7 at v = -16.6, where exp(-v) crosses 2^24, inside the derived sum
#   fp32 mode (silu_for<float>: v / (1 + expf(-v)), expf within 1 ulp, IEEE division): 2^-23 + 2^-24 + 2^-24 = 2^-22
# test_conv_ref_cpu.py checks all three against NumPy restatements whose exp2 / exp and reciprocal results are off by up to 1 ulp either way.
SILU_V_MAX = 80.0


def act_slack(v64, prec, act):
    """A(prec, act) at the activation's float64 argument v."""
    v = np.asarray(v64, np.float64)
    if act != ACT_SILU:
        assert act in (ACT_NONE, ACT_RELU, ACT_LEAKY), act
        return np.zeros_like(v)
    assert np.abs(v).max() <= SILU_V_MAX, "the SiLU bound is derived for |v| <= %g" % SILU_V_MAX
    s = np.abs(R.act_ref(v, ACT_SILU))
    if prec in ("fp16", "bf16"):
        return 2.0 ** -23 * (np.abs(v) + 3.0) * s
    if prec == "fp16x3":
        return 3 * 2.0 ** -23 * s
    if prec == "fp32":
        return 2.0 ** -22 * s
    raise ValueError(prec)


def weights_as_stored(w32, prec):
    """The float32 weights as the engine's packing stores them (see the module docstring)."""
    return R.storage_round(np.asarray(w32, np.float32), prec)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt))


def _conv64(x, w, b, stride, pad):
    return F.conv2d(_t(x, np.float64), _t(w, np.float64), None if b is None else _t(b, np.float64), stride=stride, padding=pad).numpy()


def conv_sums64(x, w, stride, pad):
    """(conv(x, w), conv(|x|, |w|)) in float64, without the bias: shared by layers that differ in their epilogue only."""
    return _conv64(x, w, None, stride, pad), _conv64(np.abs(x), np.abs(w), None, stride, pad)


def layer_from_sums(sums64, b, act, r=None, res_mode=RES_NONE):
    """The layer's float64 reference from conv_sums64.  Returns (want, S, v): v is the activation's argument."""
    assert (r is None) == (res_mode == RES_NONE)
    b64 = np.asarray(b, np.float64)[None, :, None, None]
    v, S = sums64[0] + b64, sums64[1] + np.abs(b64)
    if res_mode == RES_BEFORE_ACT:
        v = v + np.asarray(r, np.float64)
        want = R.act_ref(v, act)
    elif res_mode == RES_AFTER_ACT:
        want = R.act_ref(v, act) + np.asarray(r, np.float64)
    else:
        want = R.act_ref(v, act)
    if r is not None:
        S = S + np.abs(np.asarray(r, np.float64))
    return want, S, v


def conv_layer_ref(x, w, b, stride, pad, act, r=None, res_mode=RES_NONE):
    """The layer in float64 on NCHW / OIHW arrays (torch conv2d in float64, the activation in float64).  Returns (want, S, v)."""
    return layer_from_sums(conv_sums64(x, w, stride, pad), b, act, r, res_mode)


def _finish_f32(acc, b, act, r, res_mode):
    """Bias, residual and activation in NumPy float32 behind a float32 accumulator (b, r: shaped like acc or broadcast)."""
    v = (acc + b).astype(np.float32)
    if res_mode == RES_BEFORE_ACT:
        return R.act_f32((v + r).astype(np.float32), act)
    if res_mode == RES_AFTER_ACT:
        return (R.act_f32(v, act) + r).astype(np.float32)
    return R.act_f32(v, act)


def sample_index(shape, n=YARD_SAMPLE, seed=0):
    """A fixed sample of output elements (all of them when the output has no more than n): index arrays (frame, channel, y, x)."""
    total = int(np.prod(shape))
    flat = np.arange(total) if total <= n else np.sort(np.random.default_rng(seed).choice(total, n, replace=False))
    return np.unravel_index(flat, shape)


def acc_f32_torch(x, w, stride, pad):
    """Restatement 1: torch's float32 conv2d (no bias).  Every element."""
    return F.conv2d(_t(x, np.float32), _t(w, np.float32), None, stride=stride, padding=pad).numpy()


def acc_f32_seq(x, w, stride, pad, idx):
    """Restatement 2: acc = 0; acc = fl(acc + fl(x_k w_k)) over k in tap-major, channel-minor order (padding taps add exact zeros),
    strictly sequential, in NumPy float32, on the sampled output elements `idx` (sample_index)."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    n, co, oy, ox = idx
    N, C, H, W = x.shape
    kh, kw = w.shape[2:]
    xp = np.zeros((N, C, H + 2 * pad, W + 2 * pad), np.float32)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    acc = np.zeros(len(n), np.float32)
    for i in range(kh):
        for j in range(kw):
            xs, ws = xp[n, :, oy * stride + i, ox * stride + j].T.copy(), w[co, :, i, j].T.copy()       # (C, samples)
            for c in range(C):
                acc = acc + xs[c] * ws[c]
    assert acc.dtype == np.float32
    return acc


def conv_accs_f32(x, w, stride, pad, out_shape):
    """Both float32 accumulators of a layer: (torch's on every element, the sample's index, the sequential one on the sample)."""
    idx = sample_index(out_shape)
    return acc_f32_torch(x, w, stride, pad), idx, acc_f32_seq(x, w, stride, pad, idx)


def yardstick_from_accs(accs, b, act, r, res_mode, want, S):
    """(worst ratio, torch's, the sequential one's): |f32 - f64| / (2^-24 S) of the two restatements, bias, residual and activation in
    NumPy float32 behind each accumulator."""
    at, idx, aq = accs
    b32 = np.asarray(b, np.float32)
    r32 = None if r is None else np.asarray(r, np.float32)
    yt = R.yardstick_ratio(_finish_f32(at, b32[None, :, None, None], act, r32, res_mode), want, S)
    ys = R.yardstick_ratio(_finish_f32(aq, b32[idx[1]], act, None if r is None else r32[idx], res_mode), want[idx], S[idx])
    return max(yt, ys), yt, ys


def conv_yardstick(x, w, b, stride, pad, act, r, res_mode, want, S):
    """The yardstick of one layer on its own operands (see yardstick_from_accs)."""
    return yardstick_from_accs(conv_accs_f32(x, w, stride, pad, want.shape), b, act, r, res_mode, want, S)


def x3_dropped(x, w, stride, pad):
    """The split precision's dropped product term of every element: conv(t(x), t(w)), t(a) = X3_T |a| for |a| >= 2^-14, |a| below."""
    t = lambda a: np.where(np.abs(a) >= 2.0 ** -14, X3_T * np.abs(a), np.abs(a)).astype(np.float64)
    return _conv64(t(np.asarray(x, np.float64)), t(np.asarray(w, np.float64)), None, stride, pad)


def conv_slack(x, w, stride, pad, act, prec, S, v):
    """slack = K_CONV 2^-24 S + X3(prec) + A(prec, act) of every element."""
    slack = K_CONV * EPS32 * S + act_slack(v, prec, act)
    if prec == "fp16x3":
        slack = slack + x3_dropped(x, w, stride, pad)
    return slack


def out_prec(prec, f32_out):
    """The storage type of the layer's OUTPUT: a float32 output buffer (f32_out=True) is stored unrounded in every mode."""
    return "fp32" if f32_out else prec


def check(got, want, prec, slack, f32_out=False):
    """(ok per element, worst |err| / bound, worst |err|) with R taken for the output's storage type.  NaN / inf are never ok."""
    p = out_prec(prec, f32_out)
    w, err = R.worst(got, want, p, slack)
    return R.round_ok(got, want, p, slack), w, err


def old_criterion(got, ref, prec):
    """What tests/test_gpu_conv.py / test_gpu_x3.py assert of a layer (there against a torch float32 forward): rel-L2 <= 1e-2 (bf16),
    1.5e-3 (fp16), 3e-6 and max|d| <= 1e-4 (fp16x3), max|d| <= 1e-3 (fp32).  Returns (passes, rel-L2, max|d|)."""
    d = np.asarray(got, np.float64) - np.asarray(ref, np.float64)
    rel, mx = float(np.linalg.norm(d) / (np.linalg.norm(ref) + 1e-30)), float(np.abs(d).max())
    tol_rel, tol_max = {"bf16": (1e-2, np.inf), "fp16": (1.5e-3, np.inf), "fp16x3": (3e-6, 1e-4), "fp32": (np.inf, 1e-3)}[prec]
    return bool(np.isfinite(d).all() and rel < tol_rel and mx < tol_max), rel, mx
