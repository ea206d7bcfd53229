"""CPU tests of tests/ops_ref.py, the per-element checker of tests/test_gpu_ops_exact.py: the checker has to be trusted before the
kernels are.  round_ok must accept every correctly rounded store and reject the nearest wrong one; the float64 references must agree
with torch's own operators; the yardstick constants must cover the float32 restatements they are derived from."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops_ref as R


def _values():
    """4.5e5 float64 values: normal magnitudes, half-subnormal ones (|v| < 6.1e-5), tiny ones, and large ones up to 3e4."""
    rng = np.random.default_rng(0)
    big = rng.uniform(2048.0, 3.0e4, 50000) * rng.choice([-1.0, 1.0], 50000)
    return np.concatenate([rng.normal(0, 3, 200000), rng.normal(0, 1e-3, 100000), rng.uniform(-6e-5, 6e-5, 100000), big])


def test_values_span_the_ranges():
    v = np.abs(_values())
    assert v.size >= 100000 and (v < 6.1e-5).sum() > 50000 and (v > 2048).sum() > 10000 and v.max() <= 3.0e4 and ((v > 0.1) & (v < 10)).sum() > 100000


@pytest.mark.parametrize("prec", R.PRECISIONS)
def test_round_ok_accepts_the_correctly_rounded_store(prec):
    """float16(float32(v)), bfloat16(float32(v)) (torch) and the NumPy restatement of x3_split / x3_join, with slack = 2^-24 |v| for the
    float32 conversion in front: every element inside the bound, and the bound is tight (worst error / bound above 0.99)."""
    v = _values()
    got = R.storage_round(v.astype(np.float32), prec)
    ok = R.round_ok(got, v, prec, R.EPS32 * np.abs(v))
    assert ok.all(), (int((~ok).sum()), v[~ok][:5], got[~ok][:5])
    f32err = np.abs(v.astype(np.float32).astype(np.float64) - v)
    store_err = np.abs(got.astype(np.float64) - v) - f32err
    if prec == "fp32":
        assert (store_err <= 0).all()
        return
    ratio = float((store_err / R.store_bound(v, prec)).max())
    print("round_ok %s: worst (|round(v) - v| - f32err) / R = %.4f" % (prec, ratio))
    assert 0.99 <= ratio <= 1.0, ratio
    if prec != "fp16x3":
        u = R.ulp16(v) if prec == "fp16" else R.ulpbf(v)
        assert float((store_err / u).max()) == 0.5   # exactly half an ulp: ties exist among 4.5e5 values, nothing beyond them


def test_ulps_agree_with_numpy_spacing():
    v = _values()
    h = v.astype(np.float32).astype(np.float16)
    same = np.abs(h.astype(np.float64)) <= np.abs(v)     # rounded towards zero: same binade as v
    assert np.array_equal(R.ulp16(v)[same], np.spacing(np.abs(h[same])).astype(np.float64))
    assert R.ulp16(1.0) == 2.0 ** -10 and R.ulp16(1e-7) == 2.0 ** -24 and R.ulp16(0.0) == 2.0 ** -24 and R.ulp16(2048.0) == 2.0
    assert R.ulpbf(1.0) == 2.0 ** -7 and R.ulpbf(-3.0) == 2.0 ** -6 and R.ulpbf(0.0) == 2.0 ** -133


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_round_ok_rejects_the_neighbouring_value(prec):
    """The representable value next to the correctly rounded one (either side) is at least half an ulp away: rejected for >= 99.9 % of
    the inputs (what is left: near-ties, where the slack of the float32 conversion reaches the neighbour)."""
    v = _values()
    v32 = v.astype(np.float32)
    slack = R.EPS32 * np.abs(v)
    if prec == "fp16":
        r = v32.astype(np.float16)
        nb = [np.nextafter(r, np.float16(np.inf)).astype(np.float64), np.nextafter(r, np.float16(-np.inf)).astype(np.float64)]
    else:
        bits = torch.from_numpy(v32).to(torch.bfloat16).view(torch.int16).numpy().astype(np.int64) & 0xffff
        sign, mag = bits & 0x8000, bits & 0x7fff
        nb = []
        for step in (1, -1):
            m = np.clip(mag + step, 0, 0x7f7f)
            nb.append(((sign | m).astype(np.uint32) << 16).astype(np.uint32).view(np.float32).astype(np.float64))
    for side in nb:
        rejected = ~R.round_ok(side, v, prec, slack)
        print("round_ok %s: neighbour rejected for %.4f %%" % (prec, 100 * rejected.mean()))
        assert rejected.mean() >= 0.999


def test_round_ok_rejects_errors_of_the_split_precision():
    """fp16x3's bound is a bound of the FORMAT (2^-22 relative plus an absolute floor of 2^-26), not of one lo half's ulp: the lo half of a
    value close to its hi half has a much finer spacing, so "the neighbouring representable value" is no yardstick here.  What must be
    rejected instead: twice the bound's two terms, 2^-21 |v| + 2^-25, on either side, over the whole normal range of the hi half
    (|v| >= 2^-14) for >= 99 % of the values (the rest: the value's own rounding error points the other way and is more than 3/4 of
    the bound); 2^-24 absolute on the half-subnormal ones (their lo half alone carries the value: up to 2^-26 of rounding, the floor);
    and the plain fp16 value (hi alone)."""
    v = _values()
    got = R.storage_round(v.astype(np.float32), "fp16x3").astype(np.float64)
    slack = R.EPS32 * np.abs(v)
    n, s = np.abs(v) >= 2.0 ** -14, np.abs(v) < 2.0 ** -14
    assert ((np.abs(v) >= 2.0 ** -14) & (np.abs(v) < 2.0 ** -4)).sum() > 50000
    for sgn in (1.0, -1.0):
        rejected = ~R.round_ok(got[n] + sgn * (2.0 ** -21 * np.abs(v[n]) + 2.0 ** -25), v[n], "fp16x3", slack[n])
        print("round_ok fp16x3: 2 R off rejected for %.4f %%" % (100 * rejected.mean()))
        assert rejected.mean() >= 0.99
        assert (~R.round_ok(got[s] + sgn * 2.0 ** -24, v[s], "fp16x3", slack[s])).all()
    big = np.abs(v) >= 2.0 ** -4
    hi_only = v.astype(np.float32).astype(np.float16).astype(np.float64)
    assert (~R.round_ok(hi_only[big], v[big], "fp16x3", slack[big])).mean() > 0.99


def test_round_ok_rejects_one_part_in_2_22_in_fp32_mode():
    """fp32 mode: R = 0, the slack is everything.  With the slack of one fp32 rounding (2^-24 |v|) a result that is 2^-22 relative off
    is rejected everywhere, and the float32 rounding of v itself is accepted."""
    v = _values()
    v = v[v != 0]
    got = v.astype(np.float32).astype(np.float64)
    slack = R.EPS32 * np.abs(v)
    assert R.round_ok(got, v, "fp32", slack).all()
    assert not R.round_ok(got * (1 + 2.0 ** -22), v, "fp32", slack).any() and not R.round_ok(got * (1 - 2.0 ** -22), v, "fp32", slack).any()


def test_round_ok_rejects_bf16_truncation():
    """A bf16 store that drops the low 16 bits instead of rounding to nearest even: rejected wherever the two differ (exact float32
    inputs, no slack).  An exact tie that nearest-even rounds up is the one place where truncation is as near as rounding: those stay
    accepted, and they are rare (16 low bits equal to 0x8000)."""
    v32 = _values().astype(np.float32)
    rne, trunc = R.storage_round(v32, "bf16"), R.bf16_truncate(v32)
    differ = rne != trunc
    tie = (v32.view(np.uint32) & np.uint32(0xffff)) == np.uint32(0x8000)
    assert differ.mean() > 0.45 and tie.mean() < 1e-4
    ok = R.round_ok(trunc, v32.astype(np.float64), "bf16", 0.0)
    assert not ok[differ & ~tie].any()
    assert ok[~differ].all() and R.round_ok(rne, v32.astype(np.float64), "bf16", 0.0).all()


def test_round_ok_never_accepts_nan_or_inf():
    assert not R.round_ok(np.array([np.nan, np.inf, -np.inf]), np.array([1.0, 1.0, 1.0]), "bf16", 1e30).any()


@pytest.mark.parametrize("C", [8, 24, 48])
def test_depth2space_ref_is_conv_transpose_with_one_hot_weights(C):
    """Graph.deconv2x2: a 1x1 conv to 4C channels (rows ordered (dy, dx, c)) + depth-to-space = ConvTranspose2d(kernel 2, stride 2).  With the
    one-hot weight W[(2 dy + dx) C + c, c, dy, dx] = 1 the transposed conv IS the move."""
    rng = np.random.default_rng(C)
    t = rng.standard_normal((2, 4 * C, 3, 5))
    Wt = np.zeros((4 * C, C, 2, 2))
    for dy in range(2):
        for dx in range(2):
            for c in range(C):
                Wt[(2 * dy + dx) * C + c, c, dy, dx] = 1.0
    want = F.conv_transpose2d(torch.from_numpy(t), torch.from_numpy(Wt), stride=2).numpy()
    got = R.depth2space_ref(t)
    assert got.shape == (2, C, 6, 10) and np.array_equal(got, want)


@pytest.mark.parametrize("C,g", [(C, g) for C in (8, 24, 48) for g in (2, 3, 4, 8) if C % g == 0])
def test_shuffle_ref_is_torch_channel_shuffle(C, g):
    x = np.random.default_rng(C * 10 + g).standard_normal((2, C, 3, 5)).astype(np.float32)
    want = torch.nn.ChannelShuffle(g)(torch.from_numpy(x)).numpy()
    got = R.shuffle_ref(x, g)
    assert np.array_equal(got, want)
    cpg = C // g
    assert np.array_equal(got, x[:, [(oc % g) * cpg + oc // g for oc in range(C)]])   # the kernel's index formula (fuse_ops.hip)


@pytest.mark.parametrize("hw", [(13, 37), (3, 5), (1, 9), (20, 20), (49, 63)], ids=str)
def test_spp_identity_under_minus_inf_padding(hw):
    """engine_load.cpp (fuse_pool_chains) runs SPP's 5 / 9 / 13 pools as the SPPF chain: 9x9 = 5x5 of 5x5, 13x13 = 5x5 of 5x5 of 5x5 under -inf padding, on ragged
    maps and on maps smaller than the window."""
    x = np.random.default_rng(1).standard_normal((2, 8) + hw) - 2.0
    p5 = R.maxpool_ref(x, 5, 1, 2)
    p55 = R.maxpool_ref(p5, 5, 1, 2)
    p555 = R.maxpool_ref(p55, 5, 1, 2)
    assert np.array_equal(p55, R.maxpool_ref(x, 9, 1, 4)) and np.array_equal(p555, R.maxpool_ref(x, 13, 1, 6))
    assert (x < 0).mean() > 0.9 and (p5 < 0).mean() > 0.5      # a zero pad would win on the border ring


def test_avgpool_and_upsample_refs():
    x = np.random.default_rng(2).standard_normal((2, 8, 5, 7))
    want, S = R.avgpool_ref(x, 3, 1, 1)
    assert np.isclose(want[0, 0, 0, 0], x[0, 0, :2, :2].sum() / 9.0) and np.isclose(S[0, 0, 0, 0], np.abs(x[0, 0, :2, :2]).sum() / 9.0)
    for k, s, p in ((2, 1, 0), (3, 2, 1), (2, 2, 0), (3, 1, 1)):
        w, _ = R.avgpool_ref(x, k, s, p)
        f = R.avgpool_f32(x, k, s, p)
        assert f.shape == w.shape and np.allclose(f, w, rtol=0, atol=1e-5)
    u = R.upsample2_ref(x)
    assert u.shape == (2, 8, 10, 14) and all(np.array_equal(u[:, :, dy::2, dx::2], x) for dy in range(2) for dx in range(2))


def test_activation_refs_and_restatements_agree():
    v = np.linspace(-9, 9, 7201)
    for act in range(7):
        a, b = R.act_ref(v, act), R.act_f32(v, act)
        assert np.allclose(a, b, rtol=0, atol=2e-6), R.ACT_NAMES[act]
    assert R.act_ref(np.array([-4.0, 0.0, 7.0]), R.ACT_HSIGMOID).tolist() == [0.0, 0.5, 1.0]
    assert R.act_ref(np.array([-4.0, 1.0, 7.0]), R.ACT_HSWISH).tolist() == [0.0, 4.0 / 6.0, 7.0]
    assert R.act_ref(np.array([-4.0, 1.0, 7.0]), R.ACT_RELU6).tolist() == [0.0, 1.0, 6.0]
    assert np.allclose(R.act_ref(np.array([-4.0, 1.0]), R.ACT_LEAKY), [-0.4, 1.0])


def test_se_gate_ref_against_torch_modules():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, 16, 5, 7))
    W1, b1, W2, b2 = rng.standard_normal((4, 16, 1, 1)), rng.standard_normal(4), rng.standard_normal((16, 4, 1, 1)), rng.standard_normal(16)
    t = lambda a: torch.from_numpy(a)
    m = t(x).mean((2, 3), keepdim=True)
    want = torch.sigmoid(F.conv2d(F.silu(F.conv2d(m, t(W1), t(b1))), t(W2), t(b2))).numpy()[:, :, 0, 0]
    assert np.allclose(R.se_gate_ref(x, W1, b1, W2, b2), want, rtol=0, atol=1e-14)
    want = F.hardsigmoid(F.conv2d(F.relu(F.conv2d(m, t(W1), t(b1))), t(W2), t(b2))).numpy()[:, :, 0, 0]
    assert np.allclose(R.se_gate_ref(x, W1, b1, W2, b2, R.ACT_RELU, R.ACT_HSIGMOID), want, rtol=0, atol=1e-14)
    for ha, ga in ((R.ACT_SILU, R.ACT_NONE), (R.ACT_RELU, R.ACT_HSIGMOID)):
        assert np.allclose(R.se_gate_f32(x, W1, b1, W2, b2, ha, ga), R.se_gate_ref(x, W1, b1, W2, b2, ha, ga), rtol=0, atol=1e-5)


def test_yardstick_constants_cover_the_float32_restatement():
    """k = max(4, 4 * worst |f32 - f64| / (2^-24 S)) of the NumPy float32 restatement in the kernel's order, on inputs of the GPU tests'
    distributions (both signs, a few units wide, stored in each of the four storage types).  The figures printed here stand next to
    YARD_AVG / YARD_WSUM / YARD_SCALE in ops_ref.py, which hold the worst ratio over these inputs and the GPU cases' own."""
    rng = np.random.default_rng(7)
    worst = {"avg": 0.0, "wsum": 0.0, "scale": 0.0}
    for prec in R.PRECISIONS:
        x = [R.storage_round((rng.standard_normal((3, 16, 22, 38)) * sc).astype(np.float32), prec) for sc in (0.8, 3.3, 3.3)]
        half = R.storage_round((rng.standard_normal((3, 16, 11, 19)) * 3.3).astype(np.float32), prec)
        for k, s, p in ((2, 1, 0), (3, 2, 1), (2, 2, 0), (3, 1, 1)):
            want, S = R.avgpool_ref(x[0], k, s, p)
            worst["avg"] = max(worst["avg"], R.yardstick_ratio(R.avgpool_f32(x[0], k, s, p), want, S))
        for ins, w in (([x[1]], [1.0]), ([x[1], half], [0.6, -0.45]), ([half, x[1], x[2]], [0.37, 0.29, 0.34]), ([x[1], x[2], half], [1.0, 0.4, 0.9])):
            for act in range(7):
                want, S, _ = R.wsum_ref(ins, w, act)
                worst["wsum"] = max(worst["wsum"], R.yardstick_ratio(R.wsum_f32(ins, w, act), want, S))
        gate = rng.uniform(0.01, 0.99, (3, 16, 1, 1)).astype(np.float32)
        want = x[1].astype(np.float64) * gate.astype(np.float64)
        worst["scale"] = max(worst["scale"], R.yardstick_ratio(x[1] * gate, want, np.abs(want)))
    print("yardstick ratios: avg-pool %.3f  wsum %.3f  scale %.4f" % (worst["avg"], worst["wsum"], worst["scale"]))
    for key, yard, k in (("avg", R.YARD_AVG, R.K_AVG), ("wsum", R.YARD_WSUM, R.K_WSUM), ("scale", R.YARD_SCALE, R.K_SCALE)):
        assert 0.85 * yard <= worst[key] <= yard, (key, worst[key], yard)     # the recorded worst ratio covers these inputs, and closely
        assert k == max(4.0, 4 * yard)                                          # the rule, nothing added
