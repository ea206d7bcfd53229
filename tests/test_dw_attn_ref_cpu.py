"""CPU tests of tests/dw_attn_ref.py, the per-element checker of tests/test_gpu_dw_attn_exact.py, and of that file's graphs.  Before a kernel
is judged: the float32 restatements sit inside the recorded yardsticks (the depth-wise one inside conv_ref's YARD_CONV, the attention
ones reproduce YARD_ATT to within 15 %); a NumPy model of attention_mfma_kernel sits inside the MFMA bound with and without +-1 ulp on its
exponentials and its reciprocal; the checker REJECTS each local mistake a depth-wise or attention kernel can make, in all four
precisions, and accepts a store moved by 0.9 of a half ulp while it rejects 1.1; every graph of the GPU file plans without a device, and the
GPU file's own check functions run here on tests/graph_interp.py's float32 forward of those graphs, so a wrong case table shows up here.

The whole-tensor criterion of tests/test_gpu_v10.py (rel-L2 <= 3e-3 fp16, 2e-2 bf16, 2e-5 | 1e-5 fp32, 3e-6 | 1e-5 fp16x3) is evaluated on
every mutated tensor, and asserted to PASS where the mutation tables below say so: in bf16 on every local mutation (the corner tap, the
strip's neighbour column, the early right edge, the channel group of one strip, the swapped frames, the residual order, ReLU for SiLU on
the quiet channel; the dropped last key, the padded keys at score 0), in fp16 on the swapped frames and the quiet channel.  A depth-wise
output sums 9 to 49 products, so one wrong tap moves an element by its own magnitude and 32 such elements of 270 000 already leave a
rel-L2 of 1.6e-2.  The criterion does NOT let through
  - any mutation in fp32 and fp16x3 mode, whose tolerances sit a few roundings above float32's own error,
  - in fp16 (3e-3) the mutations that move their elements by a full magnitude: every depth-wise one but the two named above, and every
    attention one,
  - in any mode the mutations that change a whole tensor, head or query block: leaky ReLU omitted, the scale applied twice, the softmax
    over the queries, v read at the k offset, either rescale left out, the last query block reading query 0."""
import numpy as np
import pytest
import torch

import dw_attn_ref as DA
import graph_interp
import ops_ref as R
import test_gpu_dw_attn_exact as GD
from test_engine_plan_cpu import BF16, F16, F32 as PF32, SKIP, X3, plan

F32 = np.float32
M = GD.M
PREC_ID = {"fp32": PF32, "fp16": F16, "bf16": BF16, "fp16x3": X3}
NONE, SILU, RELU, LEAKY = R.ACT_NONE, R.ACT_SILU, R.ACT_RELU, R.ACT_LEAKY


# ------------------------------------------------------------------------------------------------------------------ depth-wise conv
def _dw_layer(rng, prec, c, k, hw, res, batch=3, quiet=None):
    """A synthetic layer of the GPU cases' distributions: signed activations stored in `prec`, He-scaled float32 taps (unrounded)."""
    x = R.storage_round(rng.standard_normal((batch, c) + hw).astype(F32), prec)
    w = (rng.standard_normal((c, 1, k, k)) * np.sqrt(2.0 / (k * k))).astype(F32)
    b = (rng.standard_normal(c) * 0.05).astype(F32)
    if quiet is not None:
        w[quiet] *= F32(0.02)
        b[quiet] *= F32(0.02)
    r = R.storage_round(rng.standard_normal((batch, c) + hw).astype(F32), prec) if res else None
    return x, w, b, r


def test_dw_restatement_stays_inside_the_conv_yardstick():
    """dw_f32_seq against float64 on k = 3 / 5 / 7, stride 1 / 2, every activation, with and without a residual, in all four storage
    roundings: the worst |f32 - f64| / (2^-24 S) stays at or below conv_ref.YARD_CONV, which K_CONV is four times of."""
    rng = np.random.default_rng(7)
    worst, at = 0.0, None
    for k in (3, 5, 7):
        for s in (1, 2):
            for prec in R.PRECISIONS:
                x, w, b, r = _dw_layer(rng, prec, 16, k, (24, 40), True)
                for act in (NONE, SILU, RELU, LEAKY):
                    for rr in ((r, None) if s == 1 else (None,)):
                        want, S, v = DA.dw_layer_ref(x, w, b, s, act, rr)
                        y = DA.dw_yardstick(x, w, b, s, act, rr, want, S)
                        if y > worst:
                            worst, at = y, (k, s, prec, R.ACT_NAMES[act], rr is not None)
    print("depth-wise yardstick ratio: %.3f at (k, s, prec, act, res) = %s  (YARD_CONV %.2f)" % (worst, at, DA.CR.YARD_CONV))
    assert 0.5 <= worst <= DA.CR.YARD_CONV


def test_dw_restatement_is_the_plain_loop_and_the_reference_the_expression():
    """dw_f32_seq against a scalar Python loop in the kernels' order (bias first, taps in (row, column) order) and dw_layer_ref against the
    expression written out, on a handful of elements of a stride-2 layer with an even width."""
    rng = np.random.default_rng(1)
    x, w, b, _ = _dw_layer(rng, "fp16", 8, 5, (7, 10), False)
    want, S, v = DA.dw_layer_ref(x, w, b, 2, LEAKY)
    seq = DA.dw_f32_seq(x, w, b, 2, LEAKY)
    assert want.shape == seq.shape == (3, 8, 4, 5)
    for n, c, oy, ox in ((0, 0, 0, 0), (2, 7, 3, 4), (1, 3, 0, 4), (1, 5, 3, 0), (0, 2, 2, 2)):
        acc, a64, s64 = b[c], float(b[c]), abs(float(b[c]))
        for i in range(5):
            for j in range(5):
                iy, ix = oy * 2 + i - 2, ox * 2 + j - 2
                if 0 <= iy < 7 and 0 <= ix < 10:
                    acc = F32(acc + F32(x[n, c, iy, ix] * w[c, 0, i, j]))
                    a64 += float(x[n, c, iy, ix]) * float(w[c, 0, i, j])
                    s64 += abs(float(x[n, c, iy, ix]) * float(w[c, 0, i, j]))
        assert seq[n, c, oy, ox] == np.maximum(acc, F32(0.1) * acc)
        assert abs(v[n, c, oy, ox] - a64) < 1e-13 and abs(S[n, c, oy, ox] - s64) < 1e-13 and abs(want[n, c, oy, ox] - (a64 if a64 > 0 else 0.1 * a64)) < 1e-13
    r = rng.standard_normal((3, 8, 7, 10))
    want, S2, v2 = DA.dw_layer_ref(x, w, b, 1, SILU, r)
    assert np.allclose(want, v2 / (1 + np.exp(-v2)) + r, rtol=0, atol=1e-13)          # the residual behind the activation


def test_dw_silu_term_follows_the_element_size():
    """x3s is a 4-byte type: the split precision takes the fp32 form of A here, not conv_ref's x3_silu form; the 16-bit modes take theirs."""
    v = np.linspace(-20, 20, 101)
    assert np.array_equal(DA.dw_act_slack(v, "fp16x3", SILU), DA.CR.act_slack(v, "fp32", SILU))
    assert np.array_equal(DA.dw_act_slack(v, "fp32", SILU), 2.0 ** -22 * np.abs(R.act_ref(v, SILU)))
    assert not np.array_equal(DA.dw_act_slack(v, "fp16x3", SILU), DA.CR.act_slack(v, "fp16x3", SILU))
    for p in ("fp16", "bf16"):
        assert np.array_equal(DA.dw_act_slack(v, p, SILU), DA.CR.act_slack(v, p, SILU))
    for act in (NONE, RELU, LEAKY):
        assert not DA.dw_act_slack(v, "fp16", act).any()


C_DW, HW_DW, QUIET = 40, (40, 56), 21


def _dw_base(prec, kind):
    """The two layers the mutations are applied to: "A" silu(dw3x3 s1) + r, "B" leaky(dw5x5 s2) on an even map.  Frames 1 and 2 are
    neighbours in a video (0.8 % apart).  Returns the operands, the float64 reference and the correct result as `prec` stores it."""
    rng = np.random.default_rng(11)
    k, s, act, res = (3, 1, SILU, True) if kind == "A" else (5, 2, LEAKY, False)
    x, w, b, r = _dw_layer(rng, "fp32", C_DW, k, HW_DW, res, quiet=QUIET)
    x[2] = x[1] + F32(0.008) * rng.standard_normal(x[1].shape).astype(F32)
    x = R.storage_round(x, prec)
    if r is not None:
        r = (F32(0.1) * r).astype(F32)
        r[2] = r[1] + F32(0.0008) * rng.standard_normal(r[1].shape).astype(F32)
        r = R.storage_round(r, prec)
    want, S, v = DA.dw_layer_ref(x, w, b, s, act, r)
    return dict(x=x, w=w, b=b, r=r, s=s, act=act, want=want, S=S, v=v, slack=DA.dw_slack(S, v, prec, act), good=R.storage_round(want.astype(F32), prec))


_BASES = {}


def dw_base(prec, kind):
    if (prec, kind) not in _BASES:
        _BASES[prec, kind] = _dw_base(prec, kind)
    return _BASES[prec, kind]


def _redo(B, prec, x=None, w=None, act=None, res_first=False):
    """The layer recomputed in float64 with a changed operand, activation or residual order, stored in `prec`."""
    x, w, act = B["x"] if x is None else x, B["w"] if w is None else w, B["act"] if act is None else act
    if res_first:
        want = R.act_ref(DA.dw_layer_ref(x, w, B["b"], B["s"], NONE)[0] + B["r"], act)
    else:
        want = DA.dw_layer_ref(x, w, B["b"], B["s"], act, B["r"])[0]
    return R.storage_round(want.astype(F32), prec)


def _region(B, *index):
    region = np.zeros(B["good"].shape, bool)
    region[index] = True
    return region


def mut_corner_tap(B, prec):
    """Frame 0, one 8-channel group: the tap (2, 2) is dropped for the outputs of the first row and the first column."""
    w = B["w"].copy()
    w[:, 0, 2, 2] = 0
    region = _region(B, 0, slice(8, 16), 0, slice(0, -1))            # (row 0 and column 0: there the tap (2, 2) reads a pixel of the image)
    region[0, 8:16, :-1, 0] = True
    return _redo(B, prec, w=w), region


def mut_strip_column(B, prec):
    """Frame 1, one row, 8 channels, the first four strips: the fourth output of a strip takes each tap from the column its neighbour reads
    (x shifted by one)."""
    x = np.zeros_like(B["x"])
    x[..., :-1] = B["x"][..., 1:]
    return _redo(B, prec, x=x), _region(B, 1, slice(8, 16), 17, slice(3, 16, 4))


def mut_right_edge(B, prec):
    """Layer B (stride 2, even width): the last output column reads the right-most input column as padding -- the kernel pads one column
    too early on the right, where an even width leaves the window k/2 - 1 columns of real padding.  Frame 2, one 8-channel group, ten rows."""
    x = B["x"].copy()
    x[..., -1] = 0
    return _redo(B, prec, x=x), _region(B, 2, slice(8, 16), slice(0, 10), -1)


def mut_channel_group(B, prec):
    """Frame 2, one strip (4 outputs of one row): the 8-channel group 8..15 is read from the next group (16..23)."""
    x = B["x"].copy()
    x[:, 8:16] = x[:, 16:24]
    return _redo(B, prec, x=x), _region(B, 2, slice(8, 16), 5, slice(16, 20))


def mut_frames_swapped(B, prec):
    """Frames 1 and 2 swapped on one row."""
    m = B["good"].copy()
    m[1, :, 20], m[2, :, 20] = B["good"][2, :, 20], B["good"][1, :, 20]
    return m, _region(B, slice(1, 3), slice(None), 20)


def mut_residual_order(B, prec):
    """Frame 0, two rows: silu(conv + b + r) where the layer says silu(conv + b) + r."""
    return _redo(B, prec, res_first=True), _region(B, 0, slice(None), slice(16, 18))


def mut_leaky_omitted(B, prec):
    """Layer B: LeakyReLU dropped, everywhere (what both kernels did before the fix)."""
    return _redo(B, prec, act=NONE), _region(B)


def mut_relu_for_silu(B, prec):
    """ReLU in place of SiLU on the quiet channel, everywhere in frame 1."""
    return _redo(B, prec, act=RELU), _region(B, 1, QUIET)


# name -> (mutation, layer, precisions in which the whole-tensor criterion is asserted to let it through)
DW_MUTATIONS = {
    "corner_tap": (mut_corner_tap, "A", ("bf16",)),
    "strip_column": (mut_strip_column, "A", ("bf16",)),
    "right_edge": (mut_right_edge, "B", ("bf16",)),
    "channel_group": (mut_channel_group, "A", ("bf16",)),
    "frames_swapped": (mut_frames_swapped, "A", ("fp16", "bf16")),
    "residual_order": (mut_residual_order, "A", ("bf16",)),
    "leaky_omitted": (mut_leaky_omitted, "B", ()),
    "relu_for_silu": (mut_relu_for_silu, "A", ("fp16", "bf16")),
}


def _judge(tag, name, prec, good, want, slack, m, region, op, norm_blind, local=True):
    ok0, w0, _ = DA.check(good, want, prec, slack)
    assert ok0.all() and w0 <= 1.0
    mutated = np.where(region, m, good)
    assert (mutated != good).any() and not (mutated != good)[~region].any()
    ok, w, err = DA.check(mutated, want, prec, slack)
    old_pass, rel, mx = DA.old_criterion(mutated, good, prec, op)
    print("%s %s %s: %d of %d elements changed, checker rejects %d (worst |err| / bound %.1f); rel-L2 %.2e max|d| %.2e -> old criterion %s"
          % (tag, name, prec, int((mutated != good).sum()), mutated.size, int((~ok).sum()), w, rel, mx, "passes" if old_pass else "fails"))
    assert not ok.all() and w > 1.0, "the checker must reject the mutation"
    assert ok[~region].all(), "and blame nothing outside it"
    if local:
        assert (~ok[region]).mean() > 0.5, "most of the mutated elements are individually out of bound"
    if prec in norm_blind:
        assert old_pass, "the whole-tensor criterion lets this mutation through: rel-L2 %.2e" % rel


@pytest.mark.parametrize("prec", R.PRECISIONS)
@pytest.mark.parametrize("name", list(DW_MUTATIONS))
def test_checker_rejects_wrong_depthwise_kernels(name, prec):
    """A float64-correct result stored through storage_round, one mistake applied inside `region`: the checker accepts the correct tensor,
    rejects the mutated one and blames nothing outside the region; the rel-L2 criterion of test_gpu_v10.py passes on the same tensor where
    NORM_BLIND says so."""
    fn, kind, norm_blind = DW_MUTATIONS[name]
    B = dw_base(prec, kind)
    m, region = fn(B, prec)
    _judge("dw", name, prec, B["good"], B["want"], B["slack"], m, region, "dw", norm_blind, local=name != "leaky_omitted")


# ------------------------------------------------------------------------------------------------------------------------ attention
def _qkv(rng, prec, hw, nh, sigma, batch=3, ramp=None):
    """Synthetic qkv: N(0, sigma) in every channel, stored in `prec`; ramp: a factor per token on the k channels."""
    t = rng.standard_normal((batch, nh, DA.HC, hw[0] * hw[1])) * sigma
    if ramp is not None:
        t[:, :, DA.KD:2 * DA.KD] *= ramp
    return R.storage_round(t.reshape(batch, nh * DA.HC, hw[0], hw[1]).astype(F32), prec)


YARD_ATT_CASES = [((1, 1), 1), ((9, 7), 1), ((8, 8), 2), ((5, 13), 1), ((8, 16), 2), ((3, 43), 1), ((20, 20), 4)]


def test_attention_yardstick_is_reproduced():
    """K_ATT = max(4, 4 * worst |f32 - f64| / (2^-24 (1 + Q) M)) over the online and the two-pass float32 restatements, in all four
    storage roundings, on N(0, sigma) operands (sigma 0.3 / 1 / 3, the GPU file's shapes) and on the qkv of every graph of the GPU file as
    tests/graph_interp.py computes it on the CPU.  The figures printed here stand next to YARD_ATT."""
    rng = np.random.default_rng(3)
    w1 = w2 = g1 = g2 = 0.0
    for hw, nh in YARD_ATT_CASES:
        for sigma in (0.3, 1.0, 3.0):
            for prec in R.PRECISIONS:
                qkv = _qkv(rng, prec, hw, nh, sigma, batch=2)
                _, y1, y2 = DA.attn_yardstick(qkv, nh, DA.attn_ref(qkv, nh))
                w1, w2 = max(w1, y1), max(w2, y2)
    for c in GD.ATT_CASES:
        full = _interp_qkv(c)
        for prec in R.PRECISIONS:
            qkv = R.storage_round(full, prec)
            _, y1, y2 = DA.attn_yardstick(qkv, c["nh"], DA.attn_ref(qkv, c["nh"]))
            g1, g2 = max(g1, y1), max(g2, y2)
    print("attention yardstick ratios: N(0, sigma) operands online %.3f two-pass %.3f;  the GPU file's graphs online %.3f two-pass %.3f  (YARD_ATT %.3f)"
          % (w1, w2, g1, g2, DA.YARD_ATT))
    assert 0.85 * DA.YARD_ATT <= max(w1, w2, g1, g2) <= DA.YARD_ATT, (w1, w2, g1, g2, DA.YARD_ATT)
    assert DA.K_ATT == max(4.0, 4 * DA.YARD_ATT)


_INTERP = {}


def _interp(c):
    """(fetch names, taps) of an attention case's graph on the CPU interpreter."""
    if c["id"] not in _INTERP:
        g, fetch = GD.att_graph(c)
        taps = {}
        graph_interp.run(g, GD.att_frames(c), taps)
        _INTERP[c["id"]] = (g, fetch, {n: taps[n] for n in fetch})
    return _INTERP[c["id"]]


def _interp_qkv(c):
    a = _interp(c)[2]["qkv"]
    return a[:, 8:8 + c["nh"] * DA.HC] if c["sliced"] else a


def test_attention_reference_is_the_expression():
    """attn_ref against torch's own softmax attention in float64, the way tests/test_gpu_v10.py writes it, and M, Q, V by hand on one element."""
    rng = np.random.default_rng(2)
    nh, hw = 2, (3, 5)
    qkv = rng.standard_normal((2, nh * DA.HC) + hw)
    ref = DA.attn_ref(qkv, nh)
    t = torch.from_numpy(qkv).view(2, nh, DA.HC, 15)
    q, k, v = t.split([DA.KD, DA.KD, DA.HD], dim=2)
    attn = ((q.transpose(-2, -1) @ k) * DA.SCALE).softmax(dim=-1)
    want = (v @ attn.transpose(-2, -1)).reshape(2, nh * DA.HD, 3, 5).numpy()
    assert np.allclose(ref["want"], want, rtol=0, atol=1e-13)
    b, h, i, d = 1, 1, 7, 9
    a = attn[b, h, i].numpy()
    assert abs(ref["M"][b, h * 64 + d, 1, 2] - (a * np.abs(v[b, h, d].numpy())).sum()) < 1e-13
    assert abs(ref["V"][b, h * 64 + d, 1, 2] - np.abs(v[b, h, d].numpy()).sum()) < 1e-13
    assert abs(ref["Q"][b, h, i] - DA.SCALE * (np.abs(q[b, h, :, i].numpy())[:, None] * np.abs(k[b, h].numpy())).sum(0).max()) < 1e-13
    assert (ref["M"] >= np.abs(ref["want"]) - 1e-15).all()


def _peaked_qkv(rng, prec, hw, nh):
    """|score| up to just under 80, and the best key's v near zero: the case in which P's subnormal grid (term b) decides."""
    N = hw[0] * hw[1]
    t = rng.standard_normal((2, nh, DA.HC, N))
    t[:, :, :2 * DA.KD] *= np.sqrt(75.0 / np.abs(DA.SCALE * np.einsum("bhci,bhcj->bhij", t[:, :, :DA.KD], t[:, :, DA.KD:2 * DA.KD])).max())
    best = (DA.SCALE * np.einsum("bhci,bhcj->bhij", t[:, :, :DA.KD], t[:, :, DA.KD:2 * DA.KD])).argmax(-1)
    for b in range(2):
        for h in range(nh):
            t[b, h, 2 * DA.KD:, np.unique(best[b, h])] *= 1e-3
    qkv = R.storage_round(t.reshape(2, nh * DA.HC, hw[0], hw[1]).astype(F32), prec)
    smax = np.abs(DA.attn_ref(qkv, nh)["s"]).max()
    assert 60 <= smax <= DA.SCORE_MAX, smax
    return qkv


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_mfma_model_sits_inside_its_bound(prec):
    """attn_mfma_model with correctly rounded and with +-1 ulp exponentials and reciprocal, stored in `prec`: inside the MFMA bound on
    N(0, sigma) operands, on a rising ramp and on the peaked case; and the scalar bound alone does NOT cover it (the terms are needed)."""
    rng = np.random.default_rng(5)
    worst, over_scalar = 0.0, 0
    cases = [(_qkv(rng, prec, hw, nh, sg, batch=2), nh) for hw, nh in (((5, 13), 1), ((3, 43), 1), ((20, 20), 2)) for sg in (0.3, 1.0, 3.0)]
    cases.append((_qkv(rng, prec, (3, 43), 1, 1.5, batch=2, ramp=np.linspace(0.05, 2.0, 129)), 1))
    cases += [(_peaked_qkv(rng, prec, (5, 13), 1), 1), (_peaked_qkv(rng, prec, (20, 20), 1), 1)]
    for qkv, nh in cases:
        ref = DA.attn_ref(qkv, nh)
        slack = DA.attn_slack(ref, "mfma", prec)
        for noise in (None, np.random.default_rng(6), np.random.default_rng(7)):
            got = R.storage_round(DA.attn_mfma_model(qkv, nh, prec, rng=noise), prec)
            ok, w, err = DA.check(got, ref["want"], prec, slack)
            assert ok.all(), (qkv.shape, nh, noise is not None, w, err)
            worst = max(worst, w)
            over_scalar += int((~DA.check(got, ref["want"], prec, DA.attn_slack(ref, "scalar", prec))[0]).sum())
    print("MFMA model %s: worst |err| / bound %.3f; %d elements outside the scalar bound" % (prec, worst, over_scalar))
    assert worst > 0.3 and over_scalar > 0


@pytest.mark.parametrize("prec", R.PRECISIONS)
def test_checker_accepts_both_restatements(prec):
    """Both float32 restatements, stored in `prec`, pass the scalar bound on every shape of the GPU file."""
    rng = np.random.default_rng(8)
    for hw, nh in YARD_ATT_CASES:
        qkv = _qkv(rng, prec, hw, nh, 1.5, batch=2)
        ref = DA.attn_ref(qkv, nh)
        slack = DA.attn_slack(ref, "scalar", prec)
        for f in (DA.attn_f32_online, DA.attn_f32_twopass):
            ok, w, err = DA.check(R.storage_round(f(qkv, nh), prec), ref["want"], prec, slack)
            assert ok.all() and w <= 1.0, (hw, nh, f.__name__, w)


def att64(qkv, nh, chunk=64, drop_last=False, pad_zero=False, no_acc_rescale=False, no_l_rescale=False, over_queries=False, v_at_k=None,
          block_q0=False, scale=DA.SCALE):
    """Chunked online-softmax attention in float64 with one knob per mistake."""
    hw = qkv.shape[2:]
    B, N = qkv.shape[0], hw[0] * hw[1]
    t = np.asarray(qkv, np.float64).reshape(B, nh, DA.HC, N)
    q, k, v = t[:, :, :DA.KD].copy(), t[:, :, DA.KD:2 * DA.KD], t[:, :, 2 * DA.KD:].copy()
    if v_at_k is not None:
        v[:, v_at_k] = t[:, v_at_k, DA.KD:DA.KD + DA.HD]
    if block_q0:
        q[..., (N - 1) // 64 * 64:] = q[..., :1]
    s = scale * np.einsum("bhci,bhcj->bhij", q, k)
    if over_queries:
        a = torch.softmax(torch.from_numpy(s), -2).numpy()
        return DA.to_nchw(np.einsum("bhij,bhdj->bhid", a, v), hw)
    m, l, acc = np.full((B, nh, N), -np.inf), np.zeros((B, nh, N)), np.zeros((B, nh, N, DA.HD))
    for j0 in range(0, N, chunk):
        last = j0 + chunk >= N
        nj = min(chunk, N - j0) - (1 if drop_last and last else 0)
        sc = s[..., j0:j0 + nj]
        if pad_zero and last:
            sc = np.concatenate([sc, np.zeros(sc.shape[:3] + (chunk - nj,))], -1)
        mn = np.maximum(m, sc.max(-1)) if sc.shape[-1] else m
        corr = np.exp(m - mn)
        p = np.exp(sc - mn[..., None])
        l = l * (1.0 if no_l_rescale and j0 else corr) + p.sum(-1)
        acc = acc * (1.0 if no_acc_rescale and last and j0 else corr[..., None]) + np.einsum("bhij,bhdj->bhid", p[..., :nj], v[..., j0:j0 + nj])
        m = mn
    return DA.to_nchw(acc / l[..., None], hw)


ATT_HW, ATT_NH = (10, 15), 2        # N = 150: 64 + 64 + 22 (scalar chunks), 128 + 22 (MFMA chunks)


def _att_base(prec):
    """qkv whose k grows with the token index (the maximum of most queries arrives in the last chunk), the float64 reference, both slacks
    and the correct result as `prec` stores it."""
    rng = np.random.default_rng(13)
    qkv = _qkv(rng, prec, ATT_HW, ATT_NH, 1.2, ramp=np.linspace(0.1, 1.6, 150) ** 2)
    ref = DA.attn_ref(qkv, ATT_NH)
    assert ((ref["s"].argmax(-1) >= 128).mean() > 0.5) and np.abs(ref["s"]).max() > 10
    assert np.allclose(att64(qkv, ATT_NH), ref["want"], rtol=0, atol=1e-12) and np.allclose(att64(qkv, ATT_NH, chunk=128), ref["want"], rtol=0, atol=1e-12)
    return dict(qkv=qkv, ref=ref, want=ref["want"], good=R.storage_round(ref["want"].astype(F32), prec),
                slack=DA.attn_slack(ref, DA.kernel_of(prec), prec))       # (the 16-bit modes: the wider MFMA bound -- a rejection there holds under the scalar one)


_ABASES = {}


def att_base(prec):
    if prec not in _ABASES:
        _ABASES[prec] = _att_base(prec)
    return _ABASES[prec]


def _aregion(B, *index):
    region = np.zeros(B["good"].shape, bool)
    region[index] = True
    return region


# name -> (knobs of att64, region, precisions in which the whole-tensor criterion is asserted to let it through)
ATT_MUTATIONS = {
    "last_key_dropped": (dict(drop_last=True), lambda B: _aregion(B, 0, slice(0, 64), 0), ("bf16",)),
    "padded_keys_score_0": (dict(pad_zero=True), lambda B: _aregion(B, 1, slice(0, 64)), ("bf16",)),
    "acc_not_rescaled": (dict(no_acc_rescale=True), lambda B: _aregion(B), ()),
    "l_not_rescaled": (dict(no_l_rescale=True), lambda B: _aregion(B), ()),
    "softmax_over_queries": (dict(over_queries=True), lambda B: _aregion(B), ()),
    "v_at_k_offset": (dict(v_at_k=1), lambda B: _aregion(B, slice(None), slice(64, 128)), ()),
    "last_block_reads_query_0": (dict(block_q0=True), lambda B: _aregion(B, 2, slice(None), slice(8, None)), ()),
    "scale_twice": (dict(scale=DA.SCALE * DA.SCALE), lambda B: _aregion(B), ()),
}


@pytest.mark.parametrize("prec", R.PRECISIONS)
@pytest.mark.parametrize("name", list(ATT_MUTATIONS))
def test_checker_rejects_wrong_attention_kernels(name, prec):
    knobs, region_of, norm_blind = ATT_MUTATIONS[name]
    B = att_base(prec)
    m = R.storage_round(att64(B["qkv"], ATT_NH, **knobs).astype(F32), prec)
    _judge("attention", name, prec, B["good"], B["want"], B["slack"], m, region_of(B), "attn", norm_blind, local=False)


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_half_ulp_is_the_line(prec):
    """A result moved by 0.9 of the store's half ulp passes everywhere; moved by 1.1 it fails on every element whose slack is negligible
    (under a twentieth of the half ulp).  The depth-wise layer has such elements in both 16-bit modes; the scalar attention bound has
    them in bf16 on a quiet qkv (Q below 1) -- in fp16 K_ATT 2^-24 is a tenth of half's half ulp and no element is that tight."""
    Bd = dw_base(prec, "A")
    qkv = _qkv(np.random.default_rng(17), prec, (9, 7), 1, 0.25)
    ref = DA.attn_ref(qkv, 1)
    for op, want, slack in (("attn", ref["want"], DA.attn_slack(ref, "scalar", prec)), ("dw", Bd["want"], Bd["slack"])):
        hb = R.store_bound(want, prec)
        tight = slack < hb / 20
        print("half ulp %s %s: %d of %d elements with a negligible slack" % (op, prec, int(tight.sum()), tight.size))
        assert tight.sum() >= 100 or (op, prec) == ("attn", "fp16")
        for sign in (1.0, -1.0):
            assert DA.check(want + sign * 0.9 * hb, want, prec, slack)[0].all()
            assert not DA.check(want + sign * 1.1 * hb, want, prec, slack)[0][tight].any()


# ------------------------------------------------------------------------------------------------------------------------- the plans
Z = M.ZeroWeights()


def test_every_depthwise_graph_plans_and_its_checks_run_on_the_interpreter():
    """Each depth-wise case: the graph plans in all four precisions with no op skipped or fused away, the forms follow Wo, the case
    table's coverage claims hold, and the GPU file's own check passes on graph_interp's float32 forward (under the fp32 bound)."""
    acts_of = {}
    for c in GD.DW_CASES:
        g = GD.dw_graph(c, Z)[0]
        for prec in R.PRECISIONS:
            rows = plan(g.tables(), PREC_ID[prec], GD.BATCH)[0]
            assert len(rows) == len(g.ops) and not rows[:, SKIP].any(), (c["id"], prec)
        assert GD.dw_forms(c) == (("strip", "plain") if GD.dw_out_hw(c)[1] >= 4 else ("plain",))
        g, ws, fetch, launches = GD.dw_graph(c)
        taps = {}
        graph_interp.run(g, GD.dw_frames(c), taps)
        worst = GD.check_dw(c, "fp32", ws, launches, {GD.dw_forms(c)[0]: {n: taps[n] for n in fetch}})
        assert max(worst.values()) <= 1.0
        for form in GD.dw_forms(c):
            acts_of.setdefault((c["k"], form), set()).add(c["act"])
    assert all(acts_of[k, f] == {NONE, SILU, RELU, LEAKY} for k in (3, 5, 7) for f in ("strip", "plain")), acts_of
    assert {c["c"] for c in GD.DW_CASES} >= {8, 40, 96}
    assert sorted(GD.dw_out_hw(c)[1] for c in GD.DW_CASES if GD.dw_forms(c) == ("plain",)) == [1, 3, 3]
    assert {GD.dw_out_hw(c)[1] % 4 for c in GD.DW_CASES if len(GD.dw_forms(c)) == 2} == {0, 1, 2, 3}
    pe = [c for c in GD.DW_CASES if c["kind"] == "pe"][0]
    ops = {o["name"]: o for o in GD.dw_graph(pe, Z)[0].ops}
    for h in range(GD.PE_NH):
        o = ops["test.h%d" % h]
        assert (o["ins"][0].coff, o["ins"][0].c, o["out"].coff, o["res"].coff) == (h * 128 + 64, 64, h * 64, h * 64)
        assert len({o["ins"][0].buf, o["out"].buf, o["res"].buf}) == 3


def test_every_attention_graph_plans_and_its_checks_run_on_the_interpreter():
    """Each attention case: the graph plans in all four precisions; the flat / peaked / ramp properties hold on the float32 forward
    (assert_variant inside check_att); the GPU file's own check passes on graph_interp's forward under the scalar fp32 bound."""
    for c in GD.ATT_CASES:
        g = GD.att_graph(c, Z)[0]
        for prec in R.PRECISIONS:
            rows = plan(g.tables(), PREC_ID[prec], GD.BATCH)[0]
            assert len(rows) == len(g.ops) and not rows[:, SKIP].any(), (c["id"], prec)
        g, fetch, taps = _interp(c)
        assert GD.check_att(c, "fp32", taps, "scalar") <= 1.0
        if c["sliced"]:
            att = [o for o in g.ops if o["name"] == "test"][0]
            assert att["ins"][0].coff == 8 and att["out"].coff == 16 and g.bufs[att["out"].buf][2] == c["nh"] * DA.HD + 32
    ids = [c["id"] for c in GD.ATT_CASES]
    assert set(GD.SCALAR16_CASES) <= set(ids) and sorted(c["hw"][0] * c["hw"][1] for c in GD.ATT_CASES if c["variant"] == "base" and not c["sliced"]) == [1, 63, 64, 65, 128, 129, 400]
