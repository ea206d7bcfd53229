"""GPU: the operators BETWEEN the convolutions (csrc/aux_kernels.hip, csrc/fuse_ops.hip), element by element against float64, in all four
precisions.  Every one of them is either exact (max-pool, upsample, depth-to-space, shuffle, input: a selection or a move rounds nothing)
or one store rounding away from exact (avg-pool, weighted sum, scale: fp32 arithmetic, one rounding into the storage type), so the bound
follows from IEEE arithmetic (tests/ops_ref.py: half an ulp of the storage type plus k fp32 roundings, k from a NumPy float32 yardstick),
not from what a kernel happens to produce.

Pattern: a unit graph  input -> 1x1 conv "expand" -> the operator -> 1x1 conv "tap";  the operator's INPUT and OUTPUT are both fetched
from the device and the reference is applied to the fetched input, so the comparison contains the operator and nothing else.  Batch 3.
Slice cases read `slice(8, c)` of a wider buffer and write `slice(16, c)` of a concat buffer whose guard channels on both sides were set
to 7.0 by launches in front of the operator: the guards must still be 7.0 afterwards and the operator's slice must hold no 7.0."""
import importlib

import numpy as np
import pytest

import ops_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
load_pkg()
CE = importlib.import_module("adas_amd.coreEngine")
M = importlib.import_module("adas_amd.models")

BATCH = 3
PRECS = list(R.PRECISIONS)
assert (M.ACT_NONE, M.ACT_SILU, M.ACT_RELU, M.ACT_LEAKY, M.ACT_HSWISH, M.ACT_HSIGMOID, M.ACT_RELU6) == tuple(range(7))


# ------------------------------------------------------------------------------------------------------------------------- helpers
def _graph(name, in_c, H, W, seed=11, gain=1.0):
    ws = M.SynthWeights(seed, gain=gain)
    g = M.Graph(name, in_c, H, W, ws)
    x, c3 = g.input()
    return g, ws, x, c3


def _frames(in_c, H, W, scale=1.0, seed=0):
    return (np.random.default_rng(seed).uniform(-1, 1, (BATCH, in_c, H, W)) * scale).astype(np.float32)


def _run(tmp_path, g, xin, prec, fetch):
    """Run the graph once; returns ({layer: fetched activation}, {layer: kernel label})."""
    path = str(tmp_path / (g.name + ".hipm"))
    g.save(path)
    e = CE.HipEngine(path, prec, BATCH)
    try:
        e.engine_inference(xin)
        acts = {n: e.fetch_activation(n, BATCH) for n in fetch}
        labels = {n: e.layer_kernel(e.layer_index(n), BATCH) for n in fetch}
    finally:
        e.close()
    return acts, labels


def _finish(g, y):
    z = g.conv(y, 8, 1, 1, "tap", act=M.ACT_NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")


def _wide(g, src, c, c3, name="expand", k=1, s=1, p=None, act=M.ACT_NONE, bias_fill=None, sliced=False):
    """`name`: a conv from the graph input to c channels -- or, sliced, to c + 16 channels of which the operator reads [8, 8 + c)."""
    full = g.conv(src, c + 16 if sliced else c, k, s, name, act=act, true_cin=c3, pad=p, bias_fill=bias_fill)
    return full.slice(8, c) if sliced else full


def _cut(a, c, sliced):
    """The operator's input out of the fetched `expand` activation."""
    return a[:, 8:8 + c] if sliced else a


def _guarded(g, src, c3, Ho, Wo, c, geom=(1, 1, 0)):
    """A concat buffer of 16 guard channels | c operator channels | 16 guard channels.  The guards are written in front of the operator
    (graph order = launch order) by zero-weight convs of the operator's own geometry with bias 7.0: exactly 7.0 in every storage type."""
    k, s, p = geom
    cat = g.buf(Ho, Wo, c + 32)
    for nm, off in (("guard_lo", 0), ("guard_hi", 16 + c)):
        g.conv(src, 16, k, s, nm, act=M.ACT_NONE, true_cin=c3, pad=p, out=cat.slice(off, 16), weight=np.zeros((16, c3, k, k), np.float32), bias_fill=7.0)
    return cat, cat.slice(16, c)


def _check_guards(acts, got, want, prec):
    """The guards are untouched, and no guard value is left in the operator's slice (a 7.0 there is the operator's own only where the
    reference itself lies within a store rounding of 7.0: bf16 has 32 values per unit at that magnitude)."""
    for nm in ("guard_lo", "guard_hi"):
        assert acts[nm].shape[1] == 16 and (acts[nm] == 7.0).all(), "%s: %d of %d guard elements overwritten" % (nm, int((acts[nm] != 7.0).sum()), acts[nm].size)
    left = (got == 7.0) & ~R.round_ok(np.full(want.shape, 7.0), want, prec, 7.0 * 2.0 ** -20)
    assert not left.any(), "the operator's slice still holds %d guard values" % int(left.sum())


def _exact(tag, prec, shape, got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = got != want          # (NaN != NaN: a NaN is a mismatch)
    n_bad = int(bad.sum())
    print("%s %s %s: %d mismatches of %d (exact)" % (tag, prec, shape, n_bad, got.size))
    assert n_bad == 0, (n_bad, np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _rounded(tag, prec, shape, got, want, slack, yard=None, yard_max=None):
    """Prints the case's figures, then asserts: the yardstick ratio of this case's inputs (NumPy float32 against float64, no device value
    in it) inside the recorded worst ratio that k is four times of, and every element inside its bound."""
    assert got.shape == want.shape, (got.shape, want.shape)
    ok = R.round_ok(got, want, prec, slack)
    w, err = R.worst(got, want, prec, slack)
    print("%s %s %s: worst |err| / bound %.3f (|err| %.3e)%s" % (tag, prec, shape, w, err, "" if yard is None else "  yardstick ratio %.4f" % yard))
    assert yard is None or yard <= yard_max, (yard, yard_max)
    assert ok.all(), (int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), got[~ok][:4], want[~ok][:4])


# ------------------------------------------------------------------------------------------------------------------------- max-pool
MAXPOOL_CASES = [   # k, s, p, channels, (H, W), slices
    (1, 1, 0, 40, (23, 37), False),     # the ONNX importer's channel copy
    (1, 1, 0, 8, (13, 17), True),
    (2, 2, 0, 8, (23, 37), False),      # odd extents: the floor of the output size drops a row and a column
    (2, 2, 0, 96, (40, 56), True),
    (3, 2, 1, 40, (23, 37), False),
    (3, 2, 1, 8, (40, 56), True),
    (3, 1, 1, 96, (13, 17), True),
    (5, 1, 2, 40, (23, 37), True),
    (5, 1, 2, 8, (3, 5), False),        # window larger than the map: every tap address of maxpool16_kernel<E, 5> is a clamped one somewhere
    (13, 1, 6, 40, (3, 5), False),
    (7, 1, 3, 40, (13, 17), False),     # 7, 9, 13 alone: the generic kernel in the 16-bit modes
    (9, 1, 4, 8, (40, 56), False),
    (13, 1, 6, 96, (13, 17), False),
]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("k,s,p,c,hw,sliced", MAXPOOL_CASES, ids=str)
def test_maxpool_exact(tmp_path, k, s, p, c, hw, sliced, prec):
    """Every max-pool instantiation (maxpool_kernel<T>, maxpool16_kernel<E, 2|3|5>, maxpool_x3_kernel<2|3>) bit for bit against
    torch's max-pool of the fetched input.  The input is negative almost everywhere (bias -2, no activation), so a zero pad instead of
    -inf wins the maximum on the whole border ring."""
    H, W = hw
    g, ws, x, c3 = _graph("mpunit", 3, H, W)
    a = _wide(g, x, c, c3, bias_fill=-2.0, sliced=sliced)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    fetch = ["expand", "test"]
    if sliced:
        # the guards take the pool's output size: a 1x1 conv at stride 1, a 3x3 stride-2 conv at stride 2 ((2, 2, 0) on an even map too)
        cat, out = _guarded(g, x, c3, Ho, Wo, c, geom=(1, 1, 0) if s == 1 else (3, 2, 1))
        fetch += ["guard_lo", "guard_hi"]
    else:
        cat = out = None
    y = g.maxpool(a, k, s, p, out=out, name="test")
    _finish(g, cat if sliced else y)
    acts, labels = _run(tmp_path, g, _frames(3, H, W), prec, fetch)
    xin = _cut(acts["expand"], c, sliced)
    assert labels["test"] == "maxpool_kernel", labels
    assert (xin < 0).mean() >= 0.9, "the input must be negative almost everywhere for a zero pad to show"
    want = R.maxpool_ref(xin, k, s, p).astype(np.float32)
    _exact("maxpool k%d s%d p%d c%d%s" % (k, s, p, c, " slices" if sliced else ""), prec, hw, acts["test"], want)
    if sliced:
        _check_guards(acts, acts["test"], want, prec)


def _spp_graph(form, H, W, c):
    g, ws, x, c3 = _graph("spp" + form, 3, H, W)
    cat = g.buf(H, W, 4 * c)
    if form == "chain":      # models._sppf: three 5x5 pools feeding each other into slices of one concat buffer
        g.conv(x, c, 1, 1, "expand", act=M.ACT_NONE, true_cin=c3, bias_fill=-2.0, out=cat.slice(0, c))
        for i in range(3):
            g.maxpool(cat.slice(i * c, c), 5, 1, 2, out=cat.slice((i + 1) * c, c), name="m%d" % i)
    else:                    # models.yolov7_tiny: SP 5, 9, 13 on one tensor, concatenated as [13, 9, 5, input]
        src = g.conv(x, c, 1, 1, "expand", act=M.ACT_NONE, true_cin=c3, bias_fill=-2.0, out=cat.slice(3 * c, c))
        for i, (k, off) in enumerate(((5, 2 * c), (9, c), (13, 0))):
            g.maxpool(src, k, 1, k // 2, out=cat.slice(off, c), name="m%d" % i)
    _finish(g, cat)
    return g


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hw", [(48, 64), (49, 63), (13, 37)], ids=str)
@pytest.mark.parametrize("form", ["chain", "trio"])
def test_sppf_chain_and_spp_trio_exact(tmp_path, monkeypatch, form, hw, prec):
    """The SPPF chain and the SPP 5 / 9 / 13 trio on both sides of sppf_pool3_applicable's LDS limit (3072 pixels), all three outputs
    against torch; with ADAS_NO_POOL_FUSE=1 (read when the engine is created) the separate launches give the same bits again."""
    H, W = hw
    c = 16
    fused = prec in ("fp16", "bf16") and H * W * 32 <= 96 * 1024
    res = {}
    for no_fuse in (False, True):
        if no_fuse:
            monkeypatch.setenv("ADAS_NO_POOL_FUSE", "1")
        else:
            monkeypatch.delenv("ADAS_NO_POOL_FUSE", raising=False)
        res[no_fuse] = _run(tmp_path, _spp_graph(form, H, W, c), _frames(3, H, W), prec, ["expand", "m0", "m1", "m2"])
    monkeypatch.delenv("ADAS_NO_POOL_FUSE", raising=False)
    acts, labels = res[False]
    want_labels = ["sppf_pool3_kernel"] + ["(fused into the SPPF pool launch)"] * 2 if fused else ["maxpool_kernel"] * 3
    assert [labels["m%d" % i] for i in range(3)] == want_labels, labels
    assert [res[True][1]["m%d" % i] for i in range(3)] == ["maxpool_kernel"] * 3, res[True][1]
    xin = acts["expand"]
    assert (xin < 0).mean() >= 0.9
    for i, k in enumerate((5, 9, 13)):
        # (the chain's pool i reads pool i - 1: under -inf padding that is the k = 5 + 4 i window of the input, tests/test_ops_ref_cpu.py)
        want = R.maxpool_ref(xin, k, 1, k // 2).astype(np.float32)
        _exact("spp %s m%d%s" % (form, i, " fused" if fused else ""), prec, hw, acts["m%d" % i], want)
        _exact("spp %s m%d separate launches" % (form, i), prec, hw, res[True][0]["m%d" % i], want)
    assert np.array_equal(res[True][0]["expand"], xin)


# ------------------------------------------------------------------------------------------------------------------------- moves
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c,hw,sliced", [(40, (11, 19), False), (24, (11, 19), True), (64, (3, 5), True)], ids=str)
def test_upsample2_exact(tmp_path, monkeypatch, c, hw, sliced, prec):
    """upsample2_kernel on its own (not folded into a consumer's loads): out[2y + dy][2x + dx] = in[y][x], odd half extents."""
    monkeypatch.setenv("ADAS_NO_UPSAMPLE_FOLD", "1")
    H, W = hw
    g, ws, x, c3 = _graph("upunit", 3, 2 * H, 2 * W)
    lo = _wide(g, x, c, c3, name="expand", k=3, s=2, sliced=sliced)
    fetch = ["expand", "test"]
    cat = out = None
    if sliced:
        cat, out = _guarded(g, x, c3, 2 * H, 2 * W, c)
        fetch += ["guard_lo", "guard_hi"]
    y = g.upsample2(lo, out=out, name="test")
    _finish(g, cat if sliced else y)
    acts, labels = _run(tmp_path, g, _frames(3, 2 * H, 2 * W), prec, fetch)
    xin = _cut(acts["expand"], c, sliced)
    assert labels["test"] == "upsample2_kernel" and xin.shape == (BATCH, c, H, W) and (xin > 0).any() and (xin < 0).any() and np.abs(xin).max() < 1e3
    want = R.upsample2_ref(xin)
    _exact("upsample2 c%d%s" % (c, " slices" if sliced else ""), prec, hw, acts["test"], want)
    if sliced:
        _check_guards(acts, acts["test"], want, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cout,hw,sliced", [(8, (11, 19), False), (24, (11, 19), True), (40, (3, 5), True)], ids=str)
def test_depth2space_exact(tmp_path, cout, hw, sliced, prec):
    """Graph.deconv2x2 = a 1x1 conv to 4 C channels + depth2space_kernel: the `.d2s` layer against the fetched 1x1 output rearranged
    (out[2y + dy][2x + dx][c] = in[y][x][(2 dy + dx) C + c])."""
    H, W = hw
    g, ws, x, c3 = _graph("d2sunit", 3, 2 * H, 2 * W)
    lo = g.conv(x, 16, 3, 2, "expand", act=M.ACT_NONE, true_cin=c3)
    fetch = ["up", "up.d2s"]
    cat = out = None
    if sliced:
        cat, out = _guarded(g, x, c3, 2 * H, 2 * W, cout)
        fetch += ["guard_lo", "guard_hi"]
    y = g.deconv2x2(lo, cout, "up", out=out)
    _finish(g, cat if sliced else y)
    acts, labels = _run(tmp_path, g, _frames(3, 2 * H, 2 * W), prec, fetch)
    t = acts["up"]
    assert labels["up.d2s"] == "depth2space_kernel" and t.shape == (BATCH, 4 * cout, H, W) and (t > 0).any() and (t < 0).any() and np.abs(t).max() < 1e3
    want = R.depth2space_ref(t)
    _exact("depth2space c%d%s" % (cout, " slices" if sliced else ""), prec, hw, acts["up.d2s"], want)
    if sliced:
        _check_guards(acts, acts["up.d2s"], want, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c,groups,sliced", [(24, 3, True), (24, 2, True), (24, 8, False), (48, 4, True), (48, 3, False), (64, 8, False), (64, 2, True), (48, 8, True)], ids=str)
def test_shuffle_exact(tmp_path, c, groups, sliced, prec):
    """shuffle_kernel<0|1|2> against torch's channel_shuffle on a ragged map; groups that do not divide 8 cross G8 groups in the split
    layout; groups != C / groups tells the permutation from its inverse."""
    H, W = 13, 17
    g, ws, x, c3 = _graph("shunit", 3, H, W)
    a = _wide(g, x, c, c3, sliced=sliced)
    fetch = ["expand", "test"]
    cat = out = None
    if sliced:
        cat, out = _guarded(g, x, c3, H, W, c)
        fetch += ["guard_lo", "guard_hi"]
    y = g.shuffle(a, groups, "test", out=out)
    _finish(g, cat if sliced else y)
    acts, labels = _run(tmp_path, g, _frames(3, H, W), prec, fetch)
    xin = _cut(acts["expand"], c, sliced)
    assert labels["test"] == "shuffle_kernel" and (xin > 0).any() and (xin < 0).any() and np.abs(xin).max() < 1e3
    want = R.shuffle_ref(xin, groups)
    inverse = xin[:, [(oc % (c // groups)) * groups + oc // (c // groups) for oc in range(c)]]
    assert (want != xin).mean() > 0.8, "the channels of a pixel must differ for a permutation to show"
    assert groups * groups == c or (want != inverse).mean() > 0.8, "... and for the permutation to differ from its inverse"
    _exact("shuffle c%d g%d%s" % (c, groups, " slices" if sliced else ""), prec, (H, W), acts["test"], want)
    if sliced:
        _check_guards(acts, acts["test"], want, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("in_c", [1, 3, 4])
def test_input_layer_exact(tmp_path, in_c, prec):
    """input_nchw_kernel / input_nchw_x3_kernel: channels [0, in_c) are the storage rounding of the frame (round to nearest even), channels
    [in_c, 8) exactly zero.  The frames hold half-subnormal values (below 6.1e-5) and values between 2048 and 3e4: the fine and the coarse end
    of each storage type."""
    H, W = 13, 17
    g, ws, x, c3 = _graph("inunit", in_c, H, W, gain=0.01)   # (small weights: the 1x1 conv behind stays far from the half range)
    assert c3 == in_c
    a = g.conv(x, 16, 1, 1, "expand", act=M.ACT_NONE, true_cin=c3)
    _finish(g, a)
    rng = np.random.default_rng(5)
    xin = rng.uniform(-1, 1, (BATCH, in_c, H, W))
    kind = rng.integers(0, 4, xin.shape)
    xin = np.where(kind == 1, xin * 6.0e-5, np.where(kind == 2, np.sign(xin) * rng.uniform(2048.0, 3.0e4, xin.shape), np.where(kind == 3, xin * 40.0, xin))).astype(np.float32)
    assert (np.abs(xin) < 6.1e-5).sum() > 50 and ((np.abs(xin) > 2048) & (np.abs(xin) <= 3.0e4)).sum() > 50
    acts, labels = _run(tmp_path, g, xin, prec, ["input"])
    got = acts["input"]
    assert labels["input"] == "input_nchw_kernel" and got.shape == (BATCH, 8, H, W)
    _exact("input pad channels in_c %d" % in_c, prec, (H, W), got[:, in_c:], np.zeros((BATCH, 8 - in_c, H, W), np.float32))
    if prec == "fp16x3":
        _rounded("input in_c %d" % in_c, prec, (H, W), got[:, :in_c], xin.astype(np.float64), 0.0)
    else:
        _exact("input in_c %d" % in_c, prec, (H, W), got[:, :in_c], R.storage_round(xin, prec))


# ------------------------------------------------------------------------------------------------------------------------- avg-pool
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("k,s,p,c,hw,sliced", [(2, 1, 0, 32, (160, 160), False), (2, 1, 0, 96, (23, 37), False), (3, 2, 1, 64, (40, 56), False), (2, 2, 0, 16, (20, 20), False),
                                               (3, 1, 1, 40, (13, 17), False), (3, 2, 1, 40, (40, 56), True)], ids=str)
def test_avgpool_rounded(tmp_path, k, s, p, c, hw, sliced, prec):
    """avgpool_kernel: the window's fp32 sum times 1 / k^2 (padding counted as zeros), one store rounding: half an ulp of the storage type
    plus K_AVG fp32 roundings of sum |x| / k^2."""
    H, W = hw
    g, ws, x, c3 = _graph("apunit", 3, H, W)
    a = _wide(g, x, c, c3, sliced=sliced)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    fetch = ["expand", "test"]
    cat = out = None
    if sliced:
        cat, out = _guarded(g, x, c3, Ho, Wo, c, geom=(k, s, p))
        fetch += ["guard_lo", "guard_hi"]
    y = g.avgpool(a, k, s, p, out=out, name="test")
    _finish(g, cat if sliced else y)
    acts, labels = _run(tmp_path, g, _frames(3, H, W), prec, fetch)
    xin = _cut(acts["expand"], c, sliced)
    assert labels["test"] == "avgpool_kernel" and (xin > 0).mean() > 0.2 and (xin < 0).mean() > 0.2 and np.abs(xin).max() < 1e3
    want, S = R.avgpool_ref(xin, k, s, p)
    yard = R.yardstick_ratio(R.avgpool_f32(xin, k, s, p), want, S)
    _rounded("avgpool k%d s%d p%d c%d%s" % (k, s, p, c, " slices" if sliced else ""), prec, hw, acts["test"], want, R.K_AVG * R.EPS32 * S, yard, R.YARD_AVG)
    if sliced:
        _check_guards(acts, acts["test"], want, prec)


# ------------------------------------------------------------------------------------------------------------------------- weighted sum
FW = lambda *p: [float(v) for v in M.fusion_weights(list(p))]
WSUM_CASES = [   # inputs ("f": full resolution, "h": half resolution), weights, activation, output map, channels, slices
    ("f", [1.0], M.ACT_NONE, (22, 38), 24, False),
    ("f", [1.0], M.ACT_SILU, (22, 38), 24, False),
    ("f", [1.0], M.ACT_RELU, (22, 38), 24, False),
    ("f", [1.0], M.ACT_LEAKY, (22, 38), 24, False),
    ("f", [1.0], M.ACT_HSWISH, (22, 38), 24, False),
    ("f", [1.0], M.ACT_HSIGMOID, (22, 38), 24, True),
    ("f", [1.0], M.ACT_RELU6, (22, 38), 24, True),
    ("fh", [0.6, -0.45], M.ACT_LEAKY, (22, 38), 40, False),
    ("hf", FW(0.7, 1.2), M.ACT_SILU, (6, 10), 40, True),
    ("ffh", FW(1.0, 0.4, 0.9), M.ACT_NONE, (22, 38), 24, False),
    ("fhf", [0.8, -0.5, 0.3], M.ACT_HSWISH, (6, 10), 24, False),
    ("hff", FW(0.5, 1.5, 0.25), M.ACT_RELU6, (22, 38), 24, True),
    ("ff", FW(1.0, 2.0), M.ACT_HSIGMOID, (6, 10), 8, True),
    ("hff", [1.0, -0.5, 0.25], M.ACT_SILU, (22, 38), 40, False),
    ("fhf", FW(0.3, 0.3, 0.3), M.ACT_RELU, (22, 38), 8, False),
]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form,weights,act,hw,c,sliced", WSUM_CASES, ids=["%s-%s-%dx%d-c%d%s" % (f, R.ACT_NAMES[a], hw[0], hw[1], c, "-slices" if sl else "") for f, w, a, hw, c, sl in WSUM_CASES])
def test_wsum_rounded(tmp_path, form, weights, act, hw, c, sliced, prec):
    """wsum_kernel: act(sum_i w_i x_i) with 1-3 inputs, the half-resolution input (read at (y >> 1, x >> 1), odd half extents) in each
    position, all seven activations on values below -3, inside (-3, 3) and above 6.  The fast SiLU of the 16-bit modes (v_exp_f32,
    v_rcp_f32) is allowed for inside the slack, by the yardstick of NumPy's float32 v / (1 + exp(-v)), not by a wider store bound."""
    H, W = hw
    g, ws, x, c3 = _graph("wsunit", 3, H, W)
    ins, names = [], []
    for i, f in enumerate(form):
        nm = "in%d" % i
        ins.append(_wide(g, x, c, c3, name=nm, sliced=sliced) if f == "f" else _wide(g, x, c, c3, name=nm, k=3, s=2, sliced=sliced))
        names.append(nm)
    fetch = names + ["test"]
    cat = out = None
    if sliced:
        cat, out = _guarded(g, x, c3, H, W, c)
        fetch += ["guard_lo", "guard_hi"]
    y = g.wsum(ins, weights, "test", act=act, out=out)
    _finish(g, cat if sliced else y)
    acts, labels = _run(tmp_path, g, _frames(3, H, W, scale=4.0), prec, fetch)
    xs = [_cut(acts[nm], c, sliced) for nm in names]
    assert labels["test"] == "wsum_kernel"
    for f, v in zip(form, xs):
        assert v.shape == ((BATCH, c, H, W) if f == "f" else (BATCH, c, H // 2, W // 2)) and (v > 0).any() and (v < 0).any() and np.abs(v).max() < 1e3
    want, S, pre = R.wsum_ref(xs, weights, act)
    assert (pre < -3).any() and (np.abs(pre) < 3).any() and (pre > 6).any(), "the sums must reach every branch of the activation"
    yard = R.yardstick_ratio(R.wsum_f32(xs, weights, act), want, S)
    _rounded("wsum %s %s c%d%s" % (form, R.ACT_NAMES[act], c, " slices" if sliced else ""), prec, hw, acts["test"], want, R.K_WSUM * R.EPS32 * S, yard, R.YARD_WSUM)
    if sliced:
        _check_guards(acts, acts["test"], want, prec)


# ------------------------------------------------------------------------------------------------------------------------- SE gate, scale
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form", ["silu-sigmoid", "relu-hsigmoid"])
@pytest.mark.parametrize("c,cr,hw,sliced", [(8, 1, (5, 7), False), (48, 12, (12, 20), False), (144, 6, (31, 33), False), (144, 6, (32, 32), False), (1152, 48, (8, 8), False),
                                            (32, 8, (40, 64), False), (48, 12, (12, 20), True), (24, 6, (31, 33), True), (40, 8, (32, 32), True)], ids=str)
def test_se_gate_and_scale(tmp_path, c, cr, hw, sliced, form, prec):
    """se_gate_kernel (one launch below 1024 pixels, se_partial_kernel + se_gate_kernel from there on) against float64 from the fetched
    input and the weights, per element.  The bound is the yardstick itself: four times the worst |g32 - g64| of the NumPy float32
    restatement on this case, at least 2^-22.  scale_kernel against x * gate of the FETCHED x and gate; in fp32 mode one correctly
    rounded multiply, bit for bit.  Slice cases (one- and two-launch form): x is channels [8, 8 + c) of a wider buffer (SeDev.in_coff,
    ScDev.in_coff), the scale writes channels [16, 16 + c) between guards (ScDev.out_coff)."""
    H, W = hw
    hidden_act, gate_act = (M.ACT_SILU, M.ACT_NONE) if form == "silu-sigmoid" else (M.ACT_RELU, M.ACT_HSIGMOID)
    g, ws, x, c3 = _graph("seunit", 3, H, W)
    a = _wide(g, x, c, c3, sliced=sliced)
    fetch = ["expand", "se.gate", "se.scale"]
    cat = out = None
    if sliced:
        cat, out = _guarded(g, x, c3, H, W, c)
        fetch += ["guard_lo", "guard_hi"]
    y = g.se(a, cr, "se", out=out, hidden_act=hidden_act, gate_act=gate_act)
    _finish(g, cat if sliced else y)
    gate_op = [o for o in g.ops if o["name"] == "se.gate"][0]
    assert (gate_op["res"] is not None) == (H * W >= 1024), "two launches from 1024 pixels on"
    acts, labels = _run(tmp_path, g, _frames(3, H, W, scale=2.0), prec, fetch)
    xin, gate, got = _cut(acts["expand"], c, sliced), acts["se.gate"], acts["se.scale"]
    assert labels["se.gate"] == "se_gate_kernel" and labels["se.scale"] == "scale_kernel"
    assert gate.shape == (BATCH, c, 1, 1) and (xin > 0).mean() > 0.2 and (xin < 0).mean() > 0.2 and np.abs(xin).max() < 1e3
    P = [ws.store["se.reduce.weight"], ws.store["se.reduce.bias"], ws.store["se.expand.weight"], ws.store["se.expand.bias"]]
    g64 = R.se_gate_ref(xin, *P, hidden_act, gate_act)
    g32 = R.se_gate_f32(xin, *P, hidden_act, gate_act)
    yard = float(np.abs(g32.astype(np.float64) - g64).max())
    bound = max(4 * yard, R.GATE_FLOOR)
    err = np.abs(gate[:, :, 0, 0].astype(np.float64) - g64)
    print("se_gate %s %s c%d cr%d %s%s: worst |err| / bound %.3f (|err| %.3e, yardstick %.3e, device / yardstick %.2f)"
          % (form, prec, c, cr, hw, " slices" if sliced else "", err.max() / bound, err.max(), yard, err.max() / yard if yard > 0 else float("inf")))
    assert np.isfinite(gate).all() and (err <= bound).all(), (int((err > bound).sum()), float(err.max()), bound)
    assert (g64 > 0.05).any() and (g64 < 0.95).any()
    want = xin.astype(np.float64) * gate.astype(np.float64)
    yard_s = R.yardstick_ratio(xin * gate, want, np.abs(want))
    if prec == "fp32":
        assert yard_s <= R.YARD_SCALE, yard_s
        _exact("scale c%d" % c, prec, hw, got, xin * gate)
    else:
        _rounded("scale c%d" % c, prec, hw, got, want, R.K_SCALE * R.EPS32 * np.abs(want), yard_s, R.YARD_SCALE)
    if sliced:
        _check_guards(acts, got, want, prec)
