"""Float64 references and per-element bounds of the two operators of csrc/dw_attn.hip, built on tests/ops_ref.py and tests/conv_ref.py:
the depth-wise conv  y = act(dwconv(x, w) + b) [+ r]  (dwconv_kernel<T, K>, dwconv_strip_kernel<T, K, S, 4>) and PSA's softmax attention
(attention_kernel<T>, attention_mfma_kernel<Fp16 | Bf16>).  No GPU and no project code in here: torch / NumPy only, tested by
tests/test_dw_attn_ref_cpu.py, used by tests/test_gpu_dw_attn_exact.py.  An element passes when  |got - want| <= R_prec(want) + slack,
R = ops_ref.store_bound (half an ulp of the storage type; zero in fp32 mode).  No device value enters want, a slack or a yardstick.

Depth-wise conv.  x and the residual r are the values the layer reads, exact values of the storage type (a joined fp16x3 pair fits
float32); w and b are the container's float32 arrays UNROUNDED in every precision (the loader keeps depth-wise taps in fp32 and only
transposes them), so no storage rounding is applied to them.  want = act(groups = C conv in float64 + b) + r, the kernel's only residual mode
(RES_AFTER_ACT).  slack = K_CONV 2^-24 S + A:
  S       sum |x| |w| + |b| + |r|: the magnitudes that enter the element,
  K_CONV  conv_ref's constant (four times its recorded yardstick YARD_CONV).  dw_f32_seq restates the layer in NumPy float32 the way the
          kernels run it -- the accumulator starts at the bias, the taps follow in (row, column) order, one rounding per product and one
          per add (never more accurate than the kernels' fmaf chain), activation and residual in float32 behind it -- and its worst
          |f32 - f64| / (2^-24 S) must stay at or below YARD_CONV on the CPU test's layers and on every GPU case's fetched operands
          (measured on the CPU test's layers: 4.87, k = 7 behind SiLU in fp32 mode),
  A       the activation's own error.  Zero for none, ReLU and leaky ReLU.  SiLU follows elem16.h silu_for<T>: the 16-bit types take
          v * rcp(1 + __expf(-v)), conv_ref.act_slack's 16-bit form; float AND the split precision's x3s are 4-byte types and take
          v / (1 + expf(-v)) with an IEEE division: 2^-22 |silu(v)| (conv_ref's fp32 form).  conv_ref.act_slack(..., "fp16x3", ...) states
          x3_silu, which these kernels do not call, and is not used here.
There is no X3 term: dwconv_*<x3s> joins each pair to float32 and multiplies in float32; nothing is dropped.

Attention.  For frame b, head h, query i, channel d, on the fetched qkv (per head 32 q, 32 k and 64 v channels; N = H W tokens):
  s_j = scale q_i . k_j,   a = softmax_j(s),   want = sum_j a_j v_jd          (float64; scale = float32(32^-0.5) as the container stores it)
  M = sum_j a_j |v_jd|,    Q_i = max_j scale sum_c |q_ic| |k_jc|,    V_d = sum_j |v_jd|.
An absolute error of a score is a relative error of its softmax weight, and a relative weight error eps moves the output by at most
2 eps M to first order (eps M through the numerator, eps |want| <= eps M through the denominator).
  scalar kernels (attention_kernel<float | x3s | f16s | uint16_t>: float32 arithmetic on the joined values, expf, IEEE reciprocal)
      slack = K_ATT 2^-24 (1 + Q_i) M.  The score's 32 products and adds err by a multiple of 2^-24 Q_i, exp's argument m - s_j <= 2 Q_i
      is rounded once, and the sums over the keys carry a multiple of 2^-24 M.  K_ATT is four times the worst ratio
      |f32 - f64| / (2^-24 (1 + Q_i) M) of two NumPy float32 restatements, at least 4: attn_f32_online (the kernel's order: q scaled
      first, sequential score, online softmax in 64-key chunks, sequential sums, one reciprocal) and attn_f32_twopass (scores by a float32
      matmul, the maximum, exp, a float32 matmul with v, a division).  YARD_ATT is the worst ratio over tests/test_dw_attn_ref_cpu.py's
      cases (noise operands and the GPU file's own graphs on the CPU interpreter; the figures stand at the constant below), which
      reproduces it to within 15 % below; every GPU case re-measures it on its own fetched qkv.
  MFMA kernel (attention_mfma_kernel<Fp16 | Bf16>: S = K Q^T and out^T = V^T P on the matrix cores with float32 accumulators, 128-key chunks)
      has the scalar slack -- its float32 sums are the same sums in another order -- and, term by term from its code:
      (a) P is rounded into the 16-bit B operand (E::pack2) while the denominator l sums the unrounded float32 p: every weight of the
          numerator moves by at most u relative, u = 2^-11 (fp16) | 2^-8 (bf16), the denominator not at all:  u M.
      (b) fp16 only: a p below 2^-14 lands on half's subnormal grid (spacing 2^-24): at most 2^-25 absolute per key, later multiplied by
          rescale factors <= 1 and divided by l >= 1 (the key that holds the maximum contributes exp(0) = 1):  2^-25 V_d.  bf16 has
          float32's exponent range; what happens below 2^-126 is in (c).
      (c) p = __expf(s_j - mn) = v_exp_f32(fl(fl(s_j - mn) fl(log2 e))): the subtraction U |s_j - m| absolute on the argument, the
          constant's and the product's rounding 2 U |s_j - m| (as detect_ref's fast form), v_exp_f32 within 1 ulp 2 U -- a relative error
          eta_j = 3 U (m - s_j) + 2 U of the weight, U = 2^-24.  The running maximum of an earlier chunk is no larger than the final m, so
          m - s_j bounds the argument in every chunk, and the rescale factor's own error multiplies numerator and denominator alike and
          cancels.  Through numerator and denominator:  sum_j a_j eta_j |v_jd| + |want| sum_j a_j eta_j.  Beyond m - s_j = 126 ln 2 the
          exponential is below 2^-126 and may come back as zero or as a subnormal (v_exp_f32 returns no subnormal): eta is evaluated at
          min(m - s_j, 88) and FLUSH_ATT V_d = 2^-120 V_d covers the rest.
      (d) the scale multiplies the float32 score behind the MFMA, not q: one more rounding, U |s_j| <= U Q_i on a score:  2 U Q_i M.
      The terms rest on |s| <= SCORE_MAX = 80 (asserted per call) and on "v_exp_f32 and expf return within 1 ulp", taken over from
      conv_ref.py / detect_ref.py.  attn_mfma_model restates the kernel in NumPy (float32 scores, 128-key chunks, P through storage_round,
      l from the unrounded p, exp2 and the reciprocal optionally moved to either float32 neighbour); the CPU test holds it inside the bound.
There is no arg-max and no undecidable element: the check covers every element of the output."""
import numpy as np
import torch
import torch.nn.functional as F

import conv_ref as CR
import ops_ref as R
from ops_ref import ACT_NONE, ACT_SILU, ACT_RELU, ACT_LEAKY, EPS32

F32 = np.float32
U = EPS32
KD, HD = 32, 64                           # the only sizes the kernels support
HC = 2 * KD + HD                          # channels of one head in qkv
SCALE = float(F32(KD ** -0.5))            # models.Graph.attention stores float(key_dim) ** -0.5; the engine hands it on as a float
SCORE_MAX = 80.0
FLUSH_ATT = 2.0 ** -120
LOG2E = F32(1.4426950408889634)
SCALAR_CHUNK, MFMA_CHUNK = 64, 128        # AT_CH, FA_CH of dw_attn.hip

# the worst |f32 - f64| / (2^-24 (1 + Q) M) of the two restatements over tests/test_dw_attn_ref_cpu.py's cases, all four storage roundings:
#   N(0, sigma) operands, sigma 0.3 / 1 / 3, N = 1 ... 400:                       online 3.988, two-pass 4.133
#   the qkv of every graph of tests/test_gpu_dw_attn_exact.py on the CPU interpreter:  online 105.8, two-pass 72.7 (n400-fall in bf16 rounding)
# The second line is what a float32 sum does on operands that are not zero-mean noise: v behind a SiLU layer has a mean, so the N = 400
# terms of an output share a sign and the partial sums are as large as M from the first chunk on (falling ramp: the large weights come
# first and 336 small same-signed addends are rounded against the full accumulator) -- up to N / 2 roundings of M, which (1 + Q) M does not
# scale with.  n400 itself measures 11.7, the flat cases 27, the rising ramp 34.  The constant is recorded 13 % above the worst
# measured figure (the CPU test holds it to within 15 %) because a GPU case re-measures on the qkv its own precision rounded.
YARD_ATT = 120.0
K_ATT = max(4.0, 4 * YARD_ATT)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


# ------------------------------------------------------------------------------------------------------------------ depth-wise conv
def _dw64(x, w, s):
    C, k = w.shape[0], w.shape[-1]
    return F.conv2d(_t64(x), _t64(w).reshape(C, 1, k, k), None, stride=s, padding=k // 2, groups=C).numpy()


def dw_layer_ref(x, w, b, s, act, r=None):
    """The layer in float64 on NCHW x, (C, 1, k, k) w, (C,) b and an optional residual of the output's shape.  Returns (want, S, v):
    v is the activation's argument."""
    b64 = np.asarray(b, np.float64)[None, :, None, None]
    v = _dw64(x, w, s) + b64
    S = _dw64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), s) + np.abs(b64)
    want = R.act_ref(v, act)
    if r is not None:
        want = want + np.asarray(r, np.float64)
        S = S + np.abs(np.asarray(r, np.float64))
    return want, S, v


def dw_act_slack(v64, prec, act):
    """A of the depth-wise kernels at the activation's float64 argument (module docstring)."""
    if act != ACT_SILU:
        assert act in (ACT_NONE, ACT_RELU, ACT_LEAKY), act
        return np.zeros_like(np.asarray(v64, np.float64))
    if prec in ("fp16", "bf16"):
        return CR.act_slack(v64, prec, ACT_SILU)
    assert prec in ("fp32", "fp16x3"), prec
    return CR.act_slack(v64, "fp32", ACT_SILU)          # x3s is a 4-byte type: silu_for's expf / IEEE-division branch


def dw_slack(S, v, prec, act):
    """slack = K_CONV 2^-24 S + A of every element."""
    return CR.K_CONV * EPS32 * S + dw_act_slack(v, prec, act)


def dw_f32_seq(x, w, b, s, act, r=None):
    """The layer in NumPy float32 in the kernels' order: acc = b; acc = fl(acc + fl(x w)) over the taps in (row, column) order (a tap
    outside the map adds an exact zero); the activation; + r.  Every element."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    B, C, H, W = x.shape
    k = w.shape[-1]
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = np.zeros((B, C, H + 2 * p + s, W + 2 * p + s), F32)
    xp[:, :, p:p + H, p:p + W] = x
    acc = np.broadcast_to(np.asarray(b, F32)[None, :, None, None], (B, C, Ho, Wo)).astype(F32)
    for i in range(k):
        for j in range(k):
            prod = (xp[:, :, i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s] * w[None, :, 0, i, j, None, None]).astype(F32)
            acc = (acc + prod).astype(F32)
    y = R.act_f32(acc, act)
    if r is not None:
        y = (y + np.asarray(r, F32)).astype(F32)
    assert y.dtype == F32
    return y


def dw_yardstick(x, w, b, s, act, r, want, S):
    """worst |f32 - f64| / (2^-24 S) of dw_f32_seq on the layer's own operands."""
    return R.yardstick_ratio(dw_f32_seq(x, w, b, s, act, r), want, S)


def check(got, want, prec, slack):
    """(ok per element, worst |err| / bound, worst |err|).  NaN / inf are never ok."""
    w, err = R.worst(got, want, prec, slack)
    return R.round_ok(got, want, prec, slack), w, err


def old_criterion(got, ref, prec, op):
    """What tests/test_gpu_v10.py asserts of these kernels: rel-L2 against float64 <= 2e-5 | 1e-5 (fp32: depth-wise | attention), 3e-3 (fp16),
    2e-2 (bf16), 3e-6 and max|d| < 1e-4 | 1e-5 (fp16x3).  Returns (passes, rel-L2, max|d|)."""
    d = np.asarray(got, np.float64) - np.asarray(ref, np.float64)
    rel, mx = float(np.linalg.norm(d) / (np.linalg.norm(ref) + 1e-30)), float(np.abs(d).max())
    tol, tol_max = {"dw": {"fp32": (2e-5, np.inf), "fp16": (3e-3, np.inf), "bf16": (2e-2, np.inf), "fp16x3": (3e-6, 1e-4)},
                    "attn": {"fp32": (1e-5, np.inf), "fp16": (3e-3, np.inf), "bf16": (2e-2, np.inf), "fp16x3": (1e-5, np.inf)}}[op][prec]
    return bool(np.isfinite(d).all() and rel <= tol and mx < tol_max), rel, mx


# ------------------------------------------------------------------------------------------------------------------------ attention
def split_heads(qkv, nh):
    """(q, k, v) of an NCHW qkv array: (B, nh, 32 | 32 | 64, N) views in its own dtype."""
    B, C, H, W = qkv.shape
    assert C == nh * HC, (C, nh)
    t = np.asarray(qkv).reshape(B, nh, HC, H * W)
    return t[:, :, :KD], t[:, :, KD:2 * KD], t[:, :, 2 * KD:]


def to_nchw(o, hw):
    """(B, nh, N, 64) -> (B, nh * 64, H, W): output channel h * 64 + d."""
    B, nh, N, hd = o.shape
    return np.ascontiguousarray(o.transpose(0, 1, 3, 2)).reshape(B, nh * hd, hw[0], hw[1])


def attn_ref(qkv, nh, scale=SCALE):
    """The float64 attention of an NCHW qkv array.  Returns a dict: want, M, V (NCHW, the output's shape), Q (B, nh, N), the scores s and
    the weights a (B, nh, N queries, N keys), hw."""
    hw = qkv.shape[2:]
    q, k, v = [np.asarray(t, np.float64) for t in split_heads(qkv, nh)]
    s = scale * np.einsum("bhci,bhcj->bhij", q, k)
    assert np.abs(s).max() <= SCORE_MAX, "the bound is derived for |score| <= %g" % SCORE_MAX
    Q = (scale * np.einsum("bhci,bhcj->bhij", np.abs(q), np.abs(k))).max(-1)
    a = torch.softmax(torch.from_numpy(s), -1).numpy()
    want = np.einsum("bhij,bhdj->bhid", a, v)
    M = np.einsum("bhij,bhdj->bhid", a, np.abs(v))
    V = np.broadcast_to(np.abs(v).sum(-1)[:, :, None, :], want.shape)
    return dict(want=to_nchw(want, hw), M=to_nchw(M, hw), V=to_nchw(V, hw), Q=Q, s=s, a=a, hw=hw, nh=nh, absv=np.abs(v))


def _q_nchw(ref):
    """Q_i spread over the output's channels."""
    B, nh, N = ref["Q"].shape
    return to_nchw(np.broadcast_to(ref["Q"][..., None], (B, nh, N, HD)), ref["hw"])


def kernel_of(prec, mfma=True):
    """Which attention kernel runs an aligned 16-bit qkv: the MFMA one unless ADAS_NO_ATTN_MFMA=1; fp32 and fp16x3 always the scalar one."""
    return "mfma" if mfma and prec in ("fp16", "bf16") else "scalar"


def attn_slack(ref, kernel, prec):
    """The slack of every output element (module docstring) for kernel "scalar" | "mfma"."""
    Qc = _q_nchw(ref)
    slack = K_ATT * U * (1.0 + Qc) * ref["M"]
    if kernel == "scalar":
        return slack
    assert kernel == "mfma" and prec in ("fp16", "bf16"), (kernel, prec)
    u = 2.0 ** -11 if prec == "fp16" else 2.0 ** -8
    slack = slack + u * ref["M"]                                                            # (a)
    if prec == "fp16":
        slack = slack + 2.0 ** -25 * ref["V"]                                               # (b)
    s = ref["s"]
    eta = 3 * U * np.minimum(s.max(-1, keepdims=True) - s, 88.0) + 2 * U
    ae = ref["a"] * eta
    slack = slack + to_nchw(np.einsum("bhij,bhdj->bhid", ae, ref["absv"]), ref["hw"]) \
        + np.abs(ref["want"]) * to_nchw(np.broadcast_to(ae.sum(-1)[..., None], ae.shape[:3] + (HD,)), ref["hw"]) + FLUSH_ATT * ref["V"]   # (c)
    return slack + 2 * U * Qc * ref["M"]                                                    # (d)


def attn_f32_online(qkv, nh, scale=SCALE, chunk=SCALAR_CHUNK):
    """Restatement 1, the scalar kernel's order in NumPy float32: q scaled first, the score a sequential sum over the 32 channels, online
    softmax over chunks of `chunk` keys (running maximum, denominator and accumulator rescaled once per chunk), keys added one by one,
    one reciprocal at the end.  Products and adds rounded separately."""
    hw = qkv.shape[2:]
    q, k, v = [np.asarray(t, F32) for t in split_heads(qkv, nh)]
    B, _, _, N = q.shape
    q = (q * F32(scale)).astype(F32)
    m, l, acc = np.full((B, nh, N), -np.inf, F32), np.zeros((B, nh, N), F32), np.zeros((B, nh, N, HD), F32)
    with np.errstate(under="ignore"):
        for j0 in range(0, N, chunk):
            nj = min(chunk, N - j0)
            s = np.zeros((B, nh, N, nj), F32)
            for c in range(KD):
                s = (s + (q[:, :, c, :, None] * k[:, :, c, None, j0:j0 + nj]).astype(F32)).astype(F32)
            mn = np.maximum(m, s.max(-1))
            corr = np.exp(m - mn).astype(F32)
            l, acc = (l * corr).astype(F32), (acc * corr[..., None]).astype(F32)
            p = np.exp((s - mn[..., None]).astype(F32)).astype(F32)
            for j in range(nj):
                l = (l + p[..., j]).astype(F32)
                acc = (acc + (p[..., j, None] * v[:, :, None, :, j0 + j]).astype(F32)).astype(F32)
            m = mn
        out = (acc * (F32(1) / l)[..., None]).astype(F32)
    assert out.dtype == F32
    return to_nchw(out, hw)


def attn_f32_twopass(qkv, nh, scale=SCALE):
    """Restatement 2, a plain two-pass softmax in NumPy float32: scores by a float32 matmul times the scale, the row maximum, exp, the
    row sum, a float32 matmul with v, a division."""
    hw = qkv.shape[2:]
    q, k, v = [np.asarray(t, F32) for t in split_heads(qkv, nh)]
    s = (np.matmul(np.ascontiguousarray(q.transpose(0, 1, 3, 2)), k) * F32(scale)).astype(F32)
    with np.errstate(under="ignore"):
        p = np.exp((s - s.max(-1, keepdims=True)).astype(F32)).astype(F32)
        l = p.sum(-1, dtype=F32)
        out = (np.matmul(p, np.ascontiguousarray(v.transpose(0, 1, 3, 2))) / l[..., None]).astype(F32)
    assert out.dtype == F32
    return to_nchw(out, hw)


def _att_ratio(got, ref):
    """worst |got - want| / (2^-24 (1 + Q) M); an element with M = 0 must be exact."""
    return R.yardstick_ratio(got, ref["want"], (1.0 + _q_nchw(ref)) * ref["M"])


def attn_yardstick(qkv, nh, ref, scale=SCALE):
    """(worst ratio, the online restatement's, the two-pass one's) on the case's own qkv."""
    y1, y2 = _att_ratio(attn_f32_online(qkv, nh, scale), ref), _att_ratio(attn_f32_twopass(qkv, nh, scale), ref)
    return max(y1, y2), y1, y2


def attn_mfma_model(qkv, nh, prec, scale=SCALE, rng=None):
    """attention_mfma_kernel in NumPy: float32 scores (a float32 matmul of the 16-bit operands, then the scale), 128-key chunks, p by exp2
    of fl(x fl(log2 e)) with no subnormal result, P rounded into the storage type for the second product, l from the unrounded p, one
    reciprocal, the output as float32 (the caller stores it).  rng: exp2 and the reciprocal land on either float32 neighbour of the exact
    value at random (+-1 ulp); None: correctly rounded."""
    assert prec in ("fp16", "bf16")
    hw = qkv.shape[2:]
    q, k, v = [np.asarray(t, F32) for t in split_heads(qkv, nh)]
    B, _, _, N = q.shape
    near = (lambda e: within_one_ulp(e, rng)) if rng is not None else (lambda e: np.asarray(e, np.float64).astype(F32))

    def fast_exp(x):
        t = (x * LOG2E).astype(F32)
        with np.errstate(under="ignore", over="ignore"):
            e = near(np.exp2(t.astype(np.float64)))
        return np.where(e < F32(2.0 ** -126), F32(0), e).astype(F32)

    m, l, acc = np.full((B, nh, N), -np.inf, F32), np.zeros((B, nh, N), F32), np.zeros((B, nh, N, HD), F32)
    qt = np.ascontiguousarray(q.transpose(0, 1, 3, 2))
    for j0 in range(0, N, MFMA_CHUNK):
        nj = min(MFMA_CHUNK, N - j0)
        s = (np.matmul(qt, k[..., j0:j0 + nj]) * F32(scale)).astype(F32)
        mn = np.maximum(m, s.max(-1))
        corr = fast_exp((m - mn).astype(F32))
        p = fast_exp((s - mn[..., None]).astype(F32))
        P = R.storage_round(p, prec)
        l = (l * corr + p.sum(-1, dtype=F32)).astype(F32)
        acc = ((acc * corr[..., None]).astype(F32) + np.matmul(P, np.ascontiguousarray(v[..., j0:j0 + nj].transpose(0, 1, 3, 2)))).astype(F32)
        m = mn
    inv = near(1.0 / l.astype(np.float64))
    return to_nchw((acc * inv[..., None]).astype(F32), hw)


def within_one_ulp(exact64, rng):
    """One of the two float32 neighbours of the exact value, at random per element (what "within 1 ulp" allows)."""
    with np.errstate(over="ignore", under="ignore"):
        near = np.asarray(exact64, np.float64).astype(F32)
    below = np.where(near.astype(np.float64) > exact64, np.nextafter(near, F32(-np.inf)), near).astype(F32)
    above = np.where(below.astype(np.float64) < exact64, np.nextafter(below, F32(np.inf)), below).astype(F32)
    return np.where(rng.integers(0, 2, near.shape) == 1, above, below).astype(F32)
